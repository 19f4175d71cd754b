"""24 mixtures of linear-Gaussian experts fitted at once (the flow of the reference's examples/ilr/evaluate_sinc_parallel.py,
which runs the 24 fits with joblib.Parallel): a noisy sinc, 24 random 80 % train splits, one ILR model per split
(stick-breaking gating over 100 experts, dx = dy = 1, affine experts, inputs and outputs standardised per model), all fitted
by meanfield_coordinate_descent_batched — one batched softmax pass per iteration for all 24 models.

--gibbs-iters G > 0 runs the reference job's full flow: a Gibbs warm-up of G sweeps from random labels, each model on its
own numpy stream seeded like its joblib worker (resample_batched, numpy_seeds = 0 .. fits - 1; one batched label pass per
sweep), then mean-field VI from the sampled parameters (randomize=False).

--svi-iters N > 0 runs the reference job's DEFAULT inference instead of coordinate descent (its --stochastic flow): after
the Gibbs warm-up, if one is asked for, N outer iterations of stochastic VI with minibatches of --svi-batch rows
(meanfield_stochastic_descent_batched, randomize=False, step size 0.5): per iteration one batched pass over the rows
every model drew — gathered on the device from the resident data — and one over all rows for the bounds.  Each model's numpy
stream is seeded like its joblib worker (0 .. fits - 1); the workers leave Python's `random`, which draws the minibatches,
unseeded, and here each model gets a stream of its own seeded the same way, so a run is reproducible.

--resident runs the coordinate-descent VI (after the Gibbs warm-up, if one is asked for) with the device-resident loop,
meanfield_coordinate_descent_batched_ilr: the update of the three blocks, the canonical form, the bound and the stopping rule stay
on the device between two passes; the likelihoods are drawn once, at the end.  Together with --svi-iters it runs the stochastic
flow with the device-resident SVI loop instead (meanfield_stochastic_descent_batched(resident=True,
sample_likelihood=False)): the natural-gradient step of every model runs on the device too, the minibatch indices are still
drawn on each model's Python stream.

--predict adds what the reference job is run for (its lines 196-201): ONE batched prediction of all fitted models over the
full input grid (meanfield_prediction_batched: the grid goes to the device once, each model's standardisation is applied in
the kernel), then the four curves of the reference's figure — the mean and the standard deviation across models of mu and
of std — and one summary line: the RMSE of the ensemble mean against sinc and the mean ensemble spread."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimo_amd.distributions import (TruncatedStickBreaking, CategoricalWithStickBreaking, StackedNormalWisharts,
                                    StackedGaussiansWithNormalWisharts, StackedMatrixNormalWisharts,
                                    StackedLinearGaussiansWithMatrixNormalWisharts)
from mimo_amd.engine import HipEngine
from mimo_amd.mixtures import BayesianMixtureOfLinearGaussians
from mimo_amd.mixtures.batched import (meanfield_coordinate_descent_batched, meanfield_coordinate_descent_batched_ilr,
                                        meanfield_prediction_batched, meanfield_stochastic_descent_batched, resample_batched)


def make_model(K, engine):
    dx = dy = 1
    gating = CategoricalWithStickBreaking(K, TruncatedStickBreaking(K, np.ones(K), 10. * np.ones(K)))
    basis_prior = StackedNormalWisharts(K, dx, np.zeros((K, dx)), 1e-2 * np.ones(K), np.stack(K * [np.eye(dx)]),
                                        (dx + 1.) * np.ones(K) + 1e-8)
    models_prior = StackedMatrixNormalWisharts(K, dx + 1, dy, np.zeros((K, dy, dx + 1)), np.stack(K * [1e-2 * np.eye(dx + 1)]),
                                               np.stack(K * [np.eye(dy)]), (dy + 1.) * np.ones(K) + 1e-8)
    return BayesianMixtureOfLinearGaussians(K, dx, dy, gating,
                                            StackedGaussiansWithNormalWisharts(K, dx, basis_prior, engine=engine),
                                            StackedLinearGaussiansWithMatrixNormalWisharts(K, dx + 1, dy, models_prior,
                                                                                           engine=engine),
                                            scale=True, engine=engine)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--fits", type=int, default=24)
    ap.add_argument("--experts", type=int, default=100)
    ap.add_argument("--iters", type=int, default=250)
    ap.add_argument("--gibbs-iters", type=int, default=0, help="Gibbs warm-up sweeps before VI (0: random VI start)")
    ap.add_argument("--svi-iters", type=int, default=0, help="outer iterations of stochastic VI (0: coordinate-descent VI)")
    ap.add_argument("--svi-batch", type=int, default=256, help="rows per minibatch of stochastic VI")
    ap.add_argument("--predict", action="store_true", help="one batched prediction of all models on the full input grid")
    ap.add_argument("--resident", action="store_true",
                    help="the device-resident loop of coordinate-descent VI, or with --svi-iters of stochastic VI (no "
                         "per-iteration likelihood draws)")
    args = ap.parse_args()
    rng = np.random.default_rng(1337)
    x = rng.uniform(-10., 10., size=(args.rows, 1))
    y = np.sinc(x / np.pi) + 0.1 * rng.standard_normal((args.rows, 1))
    ntrain = int(0.8 * args.rows)
    engine = HipEngine(0)
    models, data = [], []
    for _ in range(args.fits):
        idx = rng.permutation(args.rows)[:ntrain]
        m = make_model(args.experts, engine)
        m.init_transform(x[idx], y[idx])
        models.append(m)
        data.append((x[idx], y[idx]))
    t0 = time.perf_counter()
    if args.gibbs_iters > 0:
        resample_batched(models, data, init_labels='random', maxiter=args.gibbs_iters, numpy_seeds=range(args.fits))
        gibbs = time.perf_counter() - t0
        print(f"Gibbs warm-up: {args.gibbs_iters} sweeps of {args.fits} models in {gibbs:.2f} s")
    if args.svi_iters > 0:
        resident = dict(resident=True, sample_likelihood=False) if args.resident else {}
        vlbs = meanfield_stochastic_descent_batched(models, data, randomize=False, maxiter=args.svi_iters, step_size=0.5,
                                                    batch_size=args.svi_batch, numpy_seeds=range(args.fits),
                                                    python_seeds=range(args.fits), **resident)
    elif args.gibbs_iters > 0:
        descent = meanfield_coordinate_descent_batched_ilr if args.resident else meanfield_coordinate_descent_batched
        vlbs = descent(models, data, randomize=False, maxiter=args.iters, tol=1e-6)
    else:
        descent = meanfield_coordinate_descent_batched_ilr if args.resident else meanfield_coordinate_descent_batched
        vlbs = descent(models, data, randomize=True, init_rng='philox', seeds=range(args.fits), maxiter=args.iters, tol=1e-6)
    wall = time.perf_counter() - t0
    final = np.array([v[-1] for v in vlbs])
    print(f"{args.fits} fits of {ntrain} rows, K = {args.experts}: best ELBO {final.max():.2f}, median {np.median(final):.2f}, "
          f"iterations {min(map(len, vlbs))} - {max(map(len, vlbs))}, wall time {wall:.2f} s")
    if args.predict:
        t0 = time.perf_counter()
        preds = meanfield_prediction_batched(models, x, prediction='average')
        wall = time.perf_counter() - t0
        mus = np.stack([p[0] for p in preds])                   # (fits, rows, 1)
        stds = np.stack([p[2] for p in preds])
        mu_mean, mu_std = mus.mean(axis=0), mus.std(axis=0)     # the reference's four curves (evaluate_sinc_parallel.py:203-208)
        std_mean, std_std = stds.mean(axis=0), stds.std(axis=0)
        rmse = float(np.sqrt(np.mean((mu_mean - np.sinc(x / np.pi)) ** 2)))
        print(f"ensemble prediction of {args.fits} models on {args.rows} inputs in one launch ({wall * 1e3:.1f} ms): "
              f"RMSE of the ensemble mean against sinc {rmse:.4f}, mean ensemble spread {float(mu_std.mean()):.4f} "
              f"(mean predictive std {float(std_mean.mean()):.4f}, its spread {float(std_std.mean()):.4f})")


if __name__ == "__main__":
    main()
