"""One batched softmax pass (BatchedHipEngine.estep) against the B solo passes it replaces (one HipEngine per problem, its
data resident), on the same inputs, after warm-up; wall time per pass (each call returns synchronised host results) and the
largest relative difference of the outputs.  Writes <out>/bench_batched.json.

    python tools/bench_batched.py --out DIR [--reps R] [--shapes 1,2,3] [--start-only | --no-start | --svi | --predict | --nested | --resident | --resident-ilr | --resident-svi]

Also times one iteration of meanfield_coordinate_descent_batched against B solo meanfield_iteration calls at shape 1
(24 ILR models, K = 100, dx = dy = 1), split into host time and pass time.

Gibbs leg (unless --no-gibbs): per shape, one batched label pass (BatchedHipEngine.gibbs_labels, Philox, statistics on)
against the B solo HipEngine.gibbs_labels calls; and one resample_batched sweep over the 24 ILR models of shape 1 (host
uniforms) against 24 solo sweeps, with the largest difference of the sampled parameters after two seeded sweeps.

Start leg (unless --no-start): per shape, the random start of a variational fit — one BatchedHipEngine.random_resp_stats
and one BatchedHipEngine.weighted_stats (host tables) against the B solo HipEngine calls, batched and solo alternated in the
same run.  --trace-start SHAPE only runs the two batched start passes a few times (for a kernel trace of the fill kernel
and the weights mode from outside) and writes nothing.

SVI leg (--svi, on its own; writes <out>/bench_batched_svi.json): per shape, one selection pass (BatchedHipEngine.estep(rows=...):
256 random rows per problem at shapes 1 and 2, 1e5 random rows per problem at shape 3) against a plain pass on a second
engine that uploaded the selected rows contiguously — identical work, so the difference is the gather —, alternated in the
same run, outputs compared bit for bit; and one outer iteration of meanfield_stochastic_descent_batched over the 24 ILR
models of shape 1 (minibatches of 256) against 24 solo meanfield_stochastic_descent iterations.  --trace-svi SHAPE only runs
the two passes a few times (for a kernel trace from outside: the selection pass is batched_kernel<.., 4>, the plain pass
batched_kernel<.., 0>) and writes nothing.

Prediction leg (--predict, on its own; writes <out>/bench_batched_predict.json): per prediction shape, one
BatchedHipEngine.predict (standardisation in the kernel) against the B solo HipEngine.predict calls it replaces, each
uploading its own standardised rows (the uploads count: that is the path replaced), alternated in the same run, outputs
compared bit for bit.  Prediction shapes: 1. B = 24, shared N = 2500, dx = dy = 1, K = 100 (the reference job's evaluation,
diagonal variance); 2. B = 64, N_b = 1e4 own rows, dx = dy = 1, K = 4 (full covariance); 3. B = 8, N_b = 2.5e5 own rows,
dx = 8, dy = 4, K = 64, diagonal variance.  --trace-predict SHAPE only runs the batched call and the solo calls a few times
(for a kernel trace from outside: predict_batched_kernel against predict_reg_kernel) and writes nothing.

Nested leg (--nested, on its own; writes <out>/bench_batched_nested.json): wall time per outer iteration of
meanfield_coordinate_descent_nested (one shared batch of M inner mixtures) against the solo
BayesianMixtureOfMixtureOfGaussians.meanfield_coordinate_descent, same seeds, the legs alternated in one run.  Nested
shapes (--shapes 1,2): 1. M = 4, K = 4, Dz = 2, N = 400 (the scale of the reference's examples/hgmm); 2. the same at N = 1e5.

Resident leg (--resident, on its own; writes <out>/batched_resident_vi.json): wall time per iteration of the device-resident
loop, meanfield_coordinate_descent_batched(resident=True), against the host route (resident=False, sample_likelihood=False) on the
same models and the same Philox start, the two alternated in one run after warm-up: per repetition fresh models run 1 and
1 + iters iterations on each route, each run clocked from the return of the start pass (the upload — 192 MB at shape 3 — and the
start are outside the clock), the difference / iters is the repetition's figure, the median is reported (what a run does once
— priors up, state back, the write-back into the models — cancels).  The host route's iteration is split into its passes and everything else.  Also the largest relative difference of the
traces, and the device / host error ratios of one update on tests/golden/vi_update_hp.npz (tests/vi_update_fixture.py).
Resident shapes (--shapes 1,2,3): 1. shape 2 (B = 64, N_b = 1e4, Dz = 2, K = 4); 2. a GMM at the size of shape 1 (B = 24,
N_b = 1600, Dz = 2, K = 100); 3. shape 3 as GMM (B = 8, N_b = 2.5e5, Dz = 12, K = 64).

Resident ILR leg (--resident-ilr, on its own; writes <out>/batched_resident_ilr_vi.json): the resident leg's scheme for mixtures of
linear-Gaussian experts — meanfield_coordinate_descent_batched_ilr against the host route
meanfield_coordinate_descent_batched(resident=False, sample_likelihood=False) on the same ILR models and the same Philox start,
alternated, 1 and 1 + iters iterations clocked from the return of the start pass; median, minimum and maximum of the
repetitions' figures (use --reps 7), the largest relative difference of the traces, and the device / host error ratios of one
update on tests/golden/vi_ilr_update_hp.npz.  Shapes (--shapes 1,2,3): 1. B = 24, N_b = 1600, dx = dy = 1, K = 100, stick-breaking
(the reference's parallel job); 2. B = 64, N_b = 1e4, dx = dy = 1, K = 4, Dirichlet; 3. B = 8, N_b = 2.5e5, dx = 8, dy = 4, K = 64,
stick-breaking.

Resident SVI leg (--resident-svi, on its own; writes <out>/batched_resident_svi.json): the resident ILR leg's scheme for stochastic
VI — meanfield_stochastic_descent_batched(resident=True) with index_rng='host' and with index_rng='philox' against the host route
(resident=False, sample_likelihood=False) on the same ILR models, randomize=False, minibatches of 256 rows, step size 0.5, the
same numpy and Python seeds; the three alternated, 1 and 1 + iters iterations per run, each run clocked from the return of the
upload; median, minimum and maximum of the repetitions' figures (use --reps 7) and the largest relative difference between the
host route's trace and the resident one on the same indices.  Shapes (--shapes 1,2,3): those of the resident ILR leg, shape 3 at
N_b = 1e5.

Shapes: 1. B = 24, N_b = 1600, Dz = 2, K = 100 (the reference's parallel ILR example); 2. B = 64, N_b = 1e4, Dz = 2, K = 4
(restarts of the toy GMM); 3. B = 8, N_b = 2.5e5, Dz = 12, K = 64 (C4 per model)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mimo_amd.batched import BatchedHipEngine  # noqa: E402
from mimo_amd.engine import HipEngine  # noqa: E402

SHAPES = {1: (24, 1600, 2, 100), 2: (64, 10000, 2, 4), 3: (8, 250000, 12, 64)}


def inputs(B, N, D, K, seed=0):
    rng = np.random.default_rng(seed)
    Zs = [rng.standard_normal((N, D)) * 1.5 + rng.standard_normal(D) for _ in range(B)]
    A = rng.standard_normal((B, K, D, D))
    W = A @ A.transpose(0, 1, 3, 2) / D + 0.3 * np.eye(D)
    return Zs, rng.standard_normal((B, K)), rng.standard_normal((B, K, D)), W


def timed(fn, reps):
    fn()
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


def run_shape(sid, reps):
    B, N, D, K = SHAPES[sid]
    Zs, c, b, W = inputs(B, N, D, K, seed=sid)
    beng = BatchedHipEngine(0)
    beng.upload(Zs)
    solos = []
    for Z in Zs:
        e = HipEngine(0)
        e.upload(Z)
        solos.append(e)
    out = {}

    def batched():
        out["b"] = beng.estep(c, b, W)

    def solo():
        out["s"] = [e.estep(c[i], b[i], W[i]) for i, e in enumerate(solos)]

    tb = timed(batched, reps)
    ts = timed(solo, reps)
    Sb, scb = out["b"]
    err = 0.
    for i, (S1, sc1) in enumerate(out["s"]):
        for x, y in ((Sb[i].n, S1.n), (Sb[i].sx, S1.sx), (Sb[i].sxx, S1.sxx), (scb[i, :1], sc1[:1])):
            err = max(err, float(np.abs(x - y).max() / max(np.abs(y).max(), 1.)))
    # the solo passes' kernel time (the engine's event profiler)
    solos[0].profile(True)
    solos[0].profile_read(reset=True)
    for _ in range(reps):
        solos[0].estep(c[0], b[0], W[0])
    prof = solos[0].profile_read(reset=True)
    solos[0].profile(False)
    for e in solos:
        e.close()
    beng.close()
    return {"shape": sid, "B": B, "N_b": N, "Dz": D, "K": K, "batched_ms": tb, "solo_sum_ms": ts, "speedup": ts / tb,
            "max_rel_diff": err, "solo_profile": prof, "reps": reps}


def run_gibbs_shape(sid, reps):
    """One batched label pass (Philox, statistics on) against the B solo label passes."""
    B, N, D, K = SHAPES[sid]
    Zs, c, b, W = inputs(B, N, D, K, seed=sid)
    seeds = [1000 + i for i in range(B)]
    beng = BatchedHipEngine(0)
    beng.upload(Zs)
    solos = []
    for Z in Zs:
        e = HipEngine(0)
        e.upload(Z)
        solos.append(e)
    out = {}

    def batched():
        out["b"] = beng.gibbs_labels(c, b, W, seeds=seeds, sweep=1)

    def solo():
        out["s"] = [e.gibbs_labels(c[i], b[i], W[i], seed=seeds[i], sweep=1) for i, e in enumerate(solos)]

    tb = timed(batched, reps)
    ts = timed(solo, reps)
    Lb, Sb = out["b"]
    err, mismatched = 0., 0
    for i, (L1, S1) in enumerate(out["s"]):
        mismatched += int(np.sum(Lb[i] != L1))
        for x, y in ((Sb[i].n, S1.n), (Sb[i].sx, S1.sx), (Sb[i].sxx, S1.sxx)):
            err = max(err, float(np.abs(x - y).max() / max(np.abs(y).max(), 1.)))
    solos[0].profile(True)
    solos[0].profile_read(reset=True)
    for _ in range(reps):
        solos[0].gibbs_labels(c[0], b[0], W[0], seed=seeds[0], sweep=1)
    prof = solos[0].profile_read(reset=True)
    solos[0].profile(False)
    for e in solos:
        e.close()
    beng.close()
    return {"gibbs_shape": sid, "B": B, "N_b": N, "Dz": D, "K": K, "batched_ms": tb, "solo_sum_ms": ts, "speedup": ts / tb,
            "max_rel_diff": err, "labels_mismatched": mismatched, "solo_profile": prof, "reps": reps}


def timed_alternating(fa, fb, reps):
    """Medians (ms) of fa and fb, called in turn."""
    for _ in range(2):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fa()
        t1 = time.perf_counter()
        fb()
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
    return float(np.median(ta)) * 1e3, float(np.median(tb)) * 1e3


def start_tables(B, N, K, seed):
    rng = np.random.default_rng(seed)
    tables = []
    for _ in range(B):
        r = rng.random((K, N))
        r /= r.sum(axis=0)
        tables.append(r)
    return tables


def run_start_shape(sid, reps):
    """The random start: one batched random_resp_stats / weighted_stats (host tables) against the B solo calls."""
    B, N, D, K = SHAPES[sid]
    Zs = inputs(B, N, D, K, seed=sid)[0]
    tables = start_tables(B, N, K, sid)
    seeds = [1000 + i for i in range(B)]
    beng = BatchedHipEngine(0)
    beng.upload(Zs)
    solos = []
    for Z in Zs:
        e = HipEngine(0)
        e.upload(Z)
        solos.append(e)
    out = {}

    def diff(Sb, Ss):
        err = 0.
        for x, y in zip(Sb, Ss):
            for u, v in ((x.n, y.n), (x.sx, y.sx), (x.sxx, y.sxx)):
                err = max(err, float(np.abs(u - v).max() / max(np.abs(v).max(), 1.)))
        return err

    def philox_b():
        out["pb"] = beng.random_resp_stats(K, seeds)

    def philox_s():
        out["ps"] = [e.random_resp_stats(K, seeds[i]) for i, e in enumerate(solos)]

    def host_b():
        out["hb"] = beng.weighted_stats(tables)

    def host_s():
        out["hs"] = [e.weighted_stats(tables[i]) for i, e in enumerate(solos)]

    pb, ps = timed_alternating(philox_b, philox_s, reps)
    hb, hs = timed_alternating(host_b, host_s, reps)
    res = {"start_shape": sid, "B": B, "N_b": N, "Dz": D, "K": K,
           "random_resp_stats": {"batched_ms": pb, "solo_sum_ms": ps, "speedup": ps / pb, "max_rel_diff": diff(out["pb"], out["ps"])},
           "weighted_stats": {"batched_ms": hb, "solo_sum_ms": hs, "speedup": hs / hb, "max_rel_diff": diff(out["hb"], out["hs"])},
           "reps": reps}
    for e in solos:
        e.close()
    beng.close()
    return res


def trace_start(sid, reps=5):
    B, N, D, K = SHAPES[sid]
    beng = BatchedHipEngine(0)
    beng.upload(inputs(B, N, D, K, seed=sid)[0])
    for _ in range(reps):
        beng.random_resp_stats(K, [1000 + i for i in range(B)])
        beng.weighted_stats(None, K)
    beng.close()


class _SweepClock:
    """BatchedHipEngine that stamps the end of every label pass: consecutive stamps of resample_batched bound one sweep."""

    def __init__(self, eng):
        self.eng, self.stamps = eng, []

    def upload(self, arrays):
        self.eng.upload(arrays)

    def label_stats(self, *a, **k):
        out = self.eng.label_stats(*a, **k)
        self.stamps.append(time.perf_counter())
        return out

    def gibbs_labels(self, *a, **k):
        out = self.eng.gibbs_labels(*a, **k)
        self.stamps.append(time.perf_counter())
        return out


def gibbs_driver_sweep(reps):
    """One resample_batched sweep over the 24 ILR models of shape 1 against 24 solo sweeps (host uniforms)."""
    from mimo_amd.mixtures.batched import resample_batched, _resample_params
    B, N, _, K = SHAPES[1]
    engines = [HipEngine(0) for _ in range(B)]
    # outputs: two seeded sweeps from the same state, batched (numpy_seeds) against solo (numpy.random.seed before each)
    models, data = ilr_models(B, N, K, engines)
    ref, _ = ilr_models(B, N, K, engines)
    resample_batched(models, data, init_labels='random', maxiter=2, numpy_seeds=range(B))
    for i, (m, (x, y)) in enumerate(zip(ref, data)):
        np.random.seed(i)
        m.resample(x, y, init_labels='random', maxiter=2, progress_bar=False)
    err = max(float(np.abs(m.models.likelihood.As - r.models.likelihood.As).max() / max(np.abs(r.models.likelihood.As).max(), 1.))
              for m, r in zip(models, ref))
    mismatched = int(sum(np.sum(m.labels_ != r.labels_) for m, r in zip(models, ref)))
    # batched: one sweep = the host halves of the 24 models + one label pass
    clock = _SweepClock(BatchedHipEngine(0))
    resample_batched(models, data, init_labels='prior', maxiter=reps + 2, engine=clock)
    batched = float(np.median(np.diff(clock.stamps)[2:])) * 1e3
    # solo: the same sweep, model by model, each on its own engine with its data resident
    S = []
    for m, (x, y) in zip(models, data):
        eng = m._bind(*m._scaled(x, y))
        S.append(eng.label_stats(m.gating.likelihood.rvs(eng.N), K))
    t = []
    for it in range(reps + 2):
        t0 = time.perf_counter()
        for i, (m, (x, y)) in enumerate(zip(models, data)):
            eng = m._bind(*m._scaled(x, y))
            _resample_params(m, S[i], None)
            _, S[i] = m._draw_labels(eng, 'host', 0, it + 1, stats=True, return_labels=False)
        t.append(time.perf_counter() - t0)
    solo = float(np.median(t[2:])) * 1e3
    return {"gibbs_driver_shape": 1, "B": B, "batched_sweep_ms": batched, "solo_sweeps_ms": solo, "speedup": solo / batched,
            "max_rel_diff_As": err, "labels_mismatched": mismatched, "reps": reps}


class _TimedEngine:
    """BatchedHipEngine that records the wall time of every pass (each call returns synchronised host results)."""

    def __init__(self, eng):
        self.eng, self.upload_s, self.pass_s = eng, 0., []

    def upload(self, arrays):
        t0 = time.perf_counter()
        self.eng.upload(arrays)
        self.upload_s += time.perf_counter() - t0

    def estep(self, *a, **k):
        t0 = time.perf_counter()
        out = self.eng.estep(*a, **k)
        self.pass_s.append(time.perf_counter() - t0)
        return out

    # the nested driver's calls: the shared upload, and the outer step counted with the passes
    def upload_shared(self, Z, B):
        t0 = time.perf_counter()
        self.eng.upload_shared(Z, B)
        self.upload_s += time.perf_counter() - t0

    def outer_responsibilities(self, log_gating):
        t0 = time.perf_counter()
        out = self.eng.outer_responsibilities(log_gating)
        self.pass_s.append(time.perf_counter() - t0)
        return out

    def __getattr__(self, name):           # (row_off, set_structure, ...: the wrapped engine's)
        return getattr(self.eng, name)


def ilr_models(B, N, K, engines, seed=0):
    from mimo_amd.distributions import (TruncatedStickBreaking, CategoricalWithStickBreaking, StackedNormalWisharts,
                                        StackedGaussiansWithNormalWisharts, StackedMatrixNormalWisharts,
                                        StackedLinearGaussiansWithMatrixNormalWisharts)
    from mimo_amd.mixtures import BayesianMixtureOfLinearGaussians
    rng = np.random.default_rng(seed)
    models, data = [], []
    for engine in engines:
        x = rng.uniform(-10., 10., size=(N, 1))
        y = np.sinc(x / np.pi) + 0.1 * rng.standard_normal((N, 1))
        gating = CategoricalWithStickBreaking(K, TruncatedStickBreaking(K, np.ones(K), 10. * np.ones(K)))
        bp = StackedNormalWisharts(K, 1, np.zeros((K, 1)), 1e-2 * np.ones(K), np.stack(K * [np.eye(1)]), 2. * np.ones(K) + 1e-8)
        mp = StackedMatrixNormalWisharts(K, 2, 1, np.zeros((K, 1, 2)), np.stack(K * [1e-2 * np.eye(2)]), np.stack(K * [np.eye(1)]),
                                         2. * np.ones(K) + 1e-8)
        m = BayesianMixtureOfLinearGaussians(K, 1, 1, gating, StackedGaussiansWithNormalWisharts(K, 1, bp, engine=engine),
                                             StackedLinearGaussiansWithMatrixNormalWisharts(K, 2, 1, mp, engine=engine),
                                             scale=True, engine=engine)
        m.init_transform(x, y)
        models.append(m)
        data.append((x, y))
    return models, data


def driver_iteration(reps):
    """One batched driver iteration against B solo meanfield_iteration calls, shape 1."""
    from mimo_amd.mixtures.batched import meanfield_coordinate_descent_batched
    B, N, _, K = SHAPES[1]
    engines = [HipEngine(0) for _ in range(B)]          # solo: every model on its own engine, its data resident
    models, data = ilr_models(B, N, K, engines)
    teng = _TimedEngine(BatchedHipEngine(0))
    seeds = list(range(B))
    meanfield_coordinate_descent_batched(models, data, init_rng='philox', seeds=seeds, maxiter=3, tol=0., engine=teng)
    teng.upload_s, teng.pass_s = 0., []
    t0 = time.perf_counter()
    meanfield_coordinate_descent_batched(models, data, randomize=False, maxiter=reps, tol=0., sample_likelihood=True, engine=teng)
    total = time.perf_counter() - t0 - teng.upload_s - teng.pass_s[0]      # (the start pass of randomize=False is not an iteration)
    pass_ms = float(np.sum(teng.pass_s[1:])) / reps * 1e3
    batched = {"iteration_ms": total / reps * 1e3, "pass_ms": pass_ms, "host_ms": total / reps * 1e3 - pass_ms}
    # solo: the same models, one meanfield_iteration each on the model's own (single-problem) engine
    states = []
    for m, (x, y) in zip(models, data):
        eng = m._bind(*m._scaled(x, y))
        states.append((eng, eng.estep(*m.canonical_expected())[0]))
    for e in engines:
        e.profile(True)
        e.profile_read(reset=True)
    t0 = time.perf_counter()
    for _ in range(reps):
        for i, m in enumerate(models):
            x, y = data[i]
            eng = m._bind(*m._scaled(x, y))
            S, _ = m.meanfield_iteration(eng, states[i][1])
            states[i] = (eng, S)
    wall = (time.perf_counter() - t0) / reps * 1e3
    kms = sum(e.profile_read(reset=True)[0] for e in engines)
    for e in engines:
        e.profile(False)
    solo = {"iteration_ms": wall, "kernel_ms": kms / reps, "host_ms": wall - kms / reps}
    return {"driver_shape": 1, "B": B, "batched": batched, "solo": solo, "reps": reps}


SVI_ROWS = {1: 256, 2: 256, 3: 100000}


def svi_engines(sid):
    """(engine with the full batch, engine with the selected rows uploaded contiguously, c, b, W, selections)."""
    B, N, D, K = SHAPES[sid]
    Zs, c, b, W = inputs(B, N, D, K, seed=sid)
    rng = np.random.default_rng(100 + sid)
    sel = [rng.integers(0, N, size=SVI_ROWS[sid]).astype(np.int64) for _ in range(B)]
    beng, geng = BatchedHipEngine(0), BatchedHipEngine(0)
    beng.upload(Zs)
    geng.upload([Z[r] for Z, r in zip(Zs, sel)])
    return beng, geng, c, b, W, sel


def run_svi_shape(sid, reps):
    """The selection pass against a plain pass over the same rows uploaded contiguously."""
    B, N, D, K = SHAPES[sid]
    beng, geng, c, b, W, sel = svi_engines(sid)
    out = {}

    def rows_pass():
        out["r"] = beng.estep(c, b, W, rows=sel)

    def plain_pass():
        out["p"] = geng.estep(c, b, W)

    tr, tp = timed_alternating(rows_pass, plain_pass, reps)
    same = bool(np.array_equal(out["r"][1], out["p"][1], equal_nan=True)
                and all(np.array_equal(x.packed(), y.packed()) for x, y in zip(out["r"][0], out["p"][0])))
    beng.close()
    geng.close()
    return {"svi_shape": sid, "B": B, "N_b": N, "Dz": D, "K": K, "rows_per_problem": SVI_ROWS[sid], "rows_pass_ms": tr,
            "plain_pass_ms": tp, "ratio": tr / tp, "bit_identical": same, "reps": reps}


def trace_svi(sid, reps=5):
    beng, geng, c, b, W, sel = svi_engines(sid)
    for _ in range(reps):
        beng.estep(c, b, W, rows=sel)
        geng.estep(c, b, W)
    beng.close()
    geng.close()


class _TimedSviEngine(_TimedEngine):
    row_off = property(lambda self: self.eng.row_off)

    def weighted_stats(self, *a, **k):
        return self.eng.weighted_stats(*a, **k)


def svi_driver_iteration(reps, batch=256):
    """One outer iteration of batched SVI (shape 1: 24 ILR models, minibatches of 256) against 24 solo iterations."""
    from mimo_amd.mixtures.batched import meanfield_stochastic_descent_batched
    B, N, _, K = SHAPES[1]
    engines = [HipEngine(0) for _ in range(B)]          # solo: every model on its own engine (and its own minibatch engine)
    models, data = ilr_models(B, N, K, engines)
    kw = dict(randomize=False, step_size=0.5, batch_size=batch)
    teng = _TimedSviEngine(BatchedHipEngine(0))
    meanfield_stochastic_descent_batched(models, data, maxiter=3, engine=teng, **kw)
    teng.upload_s, teng.pass_s = 0., []
    t0 = time.perf_counter()
    meanfield_stochastic_descent_batched(models, data, maxiter=reps, engine=teng, **kw)
    total = (time.perf_counter() - t0 - teng.upload_s) / reps * 1e3
    pass_ms = float(np.sum(teng.pass_s)) / reps * 1e3
    batched = {"iteration_ms": total, "pass_ms": pass_ms, "rows_pass_ms": float(np.median(teng.pass_s[0::2])) * 1e3,
               "bound_pass_ms": float(np.median(teng.pass_s[1::2])) * 1e3, "host_ms": total - pass_ms}
    for m, (x, y) in zip(models, data):                  # warm-up: data resident, minibatch engines created
        m.meanfield_stochastic_descent(x, y, maxiter=3, progress_bar=False, **kw)
    t0 = time.perf_counter()
    for m, (x, y) in zip(models, data):
        m.meanfield_stochastic_descent(x, y, maxiter=reps, progress_bar=False, **kw)
    solo = (time.perf_counter() - t0) / reps * 1e3
    return {"svi_driver_shape": 1, "B": B, "batch_size": batch, "batched": batched, "solo_iterations_ms": solo,
            "speedup": solo / total, "reps": reps}


# (B, N, dx, dy, K, shared rows, variance)
PREDICT_SHAPES = {1: (24, 2500, 1, 1, 100, True, 'diagonal'), 2: (64, 10000, 1, 1, 4, False, 'full'),
                  3: (8, 250000, 8, 4, 64, False, 'diagonal')}


def predict_inputs(sid):
    B, N, dx, dy, K, shared, variance = PREDICT_SHAPES[sid]
    rng = np.random.default_rng(200 + sid)
    dc = dx + 1

    def spd(d, lead):
        A = rng.standard_normal(lead + (d, d))
        return A @ np.swapaxes(A, -1, -2) / d + 0.3 * np.eye(d)
    x = rng.standard_normal((N, dx)) * 3. + 1. if shared else [rng.standard_normal((N, dx)) * 3. + 1. for _ in range(B)]
    par = dict(c=rng.standard_normal((B, K)), b=rng.standard_normal((B, K, dx)), W=spd(dx, (B, K)),
               M=rng.standard_normal((B, K, dy, dc)), Q=0.05 * spd(dc, (B, K)), Cc=spd(dy, (B, K)))
    tf = np.stack([np.stack([rng.standard_normal(dx), 0.5 + rng.random(dx)]) for _ in range(B)])
    return x, par, tf, shared, variance


def predict_calls(sid):
    """(batched call, solo calls, results dict, close)."""
    B = PREDICT_SHAPES[sid][0]
    x, par, tf, shared, variance = predict_inputs(sid)
    beng, seng = BatchedHipEngine(0), HipEngine(0)
    out = {}

    def batched():
        out["b"] = beng.predict(x, par["c"], par["b"], par["W"], par["M"], par["Q"], par["Cc"], variance=variance, x_transform=tf)

    def solo():
        res = []
        for i in range(B):
            xi = x if shared else x[i]
            seng.upload(np.ascontiguousarray((xi - tf[i, 0]) / tf[i, 1]))
            res.append(seng.predict(*(par[k][i] for k in ("c", "b", "W", "M", "Q", "Cc")), variance=variance))
        out["s"] = res

    def close():
        beng.close()
        seng.close()
    return batched, solo, out, close


def run_predict_shape(sid, reps):
    B, N, dx, dy, K, shared, variance = PREDICT_SHAPES[sid]
    batched, solo, out, close = predict_calls(sid)
    tb, ts = timed_alternating(batched, solo, reps)
    flat = lambda r: [r[0]] + (list(r[1]) if isinstance(r[1], tuple) else [r[1]])
    same = all(np.array_equal(u, v) for rb, rs in zip(out["b"], out["s"]) for u, v in zip(flat(rb), flat(rs)))
    close()
    return {"predict_shape": sid, "B": B, "N_b": N, "dx": dx, "dy": dy, "K": K, "shared_rows": shared, "variance": variance,
            "batched_ms": tb, "solo_sum_ms": ts, "speedup": ts / tb, "bit_identical": bool(same), "reps": reps}


def trace_predict(sid, reps=5):
    batched, solo, _, close = predict_calls(sid)
    for _ in range(reps):
        batched()
        solo()
    close()


NESTED_SHAPES = {1: (4, 4, 2, 400), 2: (4, 4, 2, 100000)}      # (M, K, Dz, N): the reference's examples/hgmm scale, and a large N


def nested_model(M, K, D, engines, seed):
    """A mixture of mixtures built as tests/model_checks.py::check_hier_gmm builds it; engines: one per inner mixture."""
    import numpy.random as npr
    from mimo_amd.distributions import (NormalWishart, TiedGaussiansWithScaledPrecision, Dirichlet, CategoricalWithDirichlet,
                                        TiedGaussiansWithHierarchicalNormalWisharts)
    from mimo_amd.mixtures import BayesianMixtureOfGaussiansWithHierarchicalPrior, BayesianMixtureOfMixtureOfGaussians
    npr.seed(seed)

    def inner(eng):
        gating = CategoricalWithDirichlet(dim=K, prior=Dirichlet(dim=K, alphas=np.ones((K,))))
        hyper = NormalWishart(dim=D, mu=np.zeros((D,)), kappa=1e-2, psi=np.eye(D), nu=D + 1. + 1e-8)
        prior = TiedGaussiansWithScaledPrecision(size=K, dim=D, kappas=1e-2 * np.ones((K,)))
        comps = TiedGaussiansWithHierarchicalNormalWisharts(size=K, dim=D, hyper_prior=hyper, prior=prior, engine=eng)
        return BayesianMixtureOfGaussiansWithHierarchicalPrior(size=K, dim=D, gating=gating, components=comps, engine=eng)
    gating = CategoricalWithDirichlet(dim=M, prior=Dirichlet(dim=M, alphas=np.ones((M,))))
    return BayesianMixtureOfMixtureOfGaussians(cluster_size=M, mixture_size=K, dim=D, gating=gating,
                                               components=[inner(e) for e in engines])


def run_nested_shape(sid, reps, iters=10):
    """Wall time per OUTER iteration of meanfield_coordinate_descent_nested against the solo
    BayesianMixtureOfMixtureOfGaussians.meanfield_coordinate_descent (one engine per inner mixture, and one engine shared by
    all of them): per repetition a fresh model from the same seeds runs 1 and 1 + iters outer iterations (randomize=False:
    every iteration is a lockstep iteration); the difference / iters is the repetition's figure, the median over the
    repetitions is reported.  Every call returns synchronised host results.  Also the largest relative difference of the
    posteriors after 1 + iters iterations."""
    import numpy.random as npr
    from mimo_amd.mixtures.batched import meanfield_coordinate_descent_nested
    M, K, D, N = NESTED_SHAPES[sid]
    rng = np.random.default_rng(sid)
    centres = rng.standard_normal((M * K, D)) * 6.0
    X = np.ascontiguousarray(centres[rng.integers(M * K, size=N)] + rng.standard_normal((N, D)))
    own, shared, beng = [HipEngine(0) for _ in range(M)], [HipEngine(0)] * M, BatchedHipEngine(0)

    def nested(n, out=None):
        mm = nested_model(M, K, D, own, 11)
        npr.seed(12)
        t0 = time.perf_counter()
        meanfield_coordinate_descent_nested(mm, X, randomize=False, maxiter=n, engine=beng)
        dt = time.perf_counter() - t0
        if out is not None:
            out.append(mm)
        return dt

    def solo(engines):
        def run(n, out=None):
            mm = nested_model(M, K, D, engines, 11)
            npr.seed(12)
            t0 = time.perf_counter()
            mm.meanfield_coordinate_descent(X, randomize=False, maxiter=n, progress_bar=False)
            dt = time.perf_counter() - t0
            if out is not None:
                out.append(mm)
            return dt
        return run
    legs = {"nested": nested, "solo_own_engines": solo(own), "solo_shared_engine": solo(shared)}
    kept = {name: [] for name in legs}
    for name, fn in legs.items():                        # warm-up, and the models the outputs are compared on
        fn(1)
        fn(1 + iters, kept[name])
    per = {name: [] for name in legs}
    for _ in range(reps):                                # the legs alternate within a repetition
        for name, fn in legs.items():
            per[name].append((fn(1 + iters) - fn(1)) / iters)

    def post(mm):
        return [mm.gating.posterior.alphas] + [c.components.posterior.mus for c in mm.components] \
            + [c.components.hyper_posterior.wishart.psi for c in mm.components] + [c.gating.posterior.alphas for c in mm.components]
    diff = max(float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
               for a, b in zip(post(kept["nested"][0]), post(kept["solo_own_engines"][0])))
    res = {"nested_shape": sid, "M": M, "K": K, "Dz": D, "N": N, "iters_per_figure": iters, "reps": reps,
           "max_rel_diff_posteriors": diff}
    for name in legs:
        res[name + "_ms_per_outer_iteration"] = float(np.median(per[name])) * 1e3
    res["speedup_vs_own_engines"] = res["solo_own_engines_ms_per_outer_iteration"] / res["nested_ms_per_outer_iteration"]
    res["speedup_vs_shared_engine"] = res["solo_shared_engine_ms_per_outer_iteration"] / res["nested_ms_per_outer_iteration"]
    # where the nested iteration's time goes: its engine calls against everything else (host updates, canonical forms)
    teng = _TimedEngine(beng)
    mm = nested_model(M, K, D, own, 11)
    npr.seed(12)
    t0 = time.perf_counter()
    meanfield_coordinate_descent_nested(mm, X, randomize=False, maxiter=1 + iters, engine=teng)
    total = time.perf_counter() - t0
    res["nested_engine_calls_ms_per_outer_iteration"] = float(np.sum(teng.pass_s)) / (1 + iters) * 1e3
    res["nested_total_ms_per_outer_iteration_with_start"] = total / (1 + iters) * 1e3
    res["nested_engine_calls_per_outer_iteration"] = len(teng.pass_s) / (1 + iters)
    return res


RESIDENT_SHAPES = {1: (64, 10000, 2, 4), 2: (24, 1600, 2, 100), 3: (8, 250000, 12, 64)}      # (B, N_b, Dz, K)


def gmm_models(B, N, D, K, engine, seed):
    """B mixtures of Gaussians (Dirichlet gating, untied Normal-Wishart components) on clustered data -> (build, data)."""
    from mimo_amd.distributions import Dirichlet, CategoricalWithDirichlet, StackedNormalWisharts, StackedGaussiansWithNormalWisharts
    from mimo_amd.mixtures import BayesianMixtureOfGaussians
    rng = np.random.default_rng(seed)
    data = []
    for _ in range(B):
        centres = rng.standard_normal((K, D)) * 4.0
        data.append(np.ascontiguousarray(centres[rng.integers(K, size=N)] + rng.standard_normal((N, D))))

    def build():
        models = []
        for _ in range(B):
            gating = CategoricalWithDirichlet(dim=K, prior=Dirichlet(dim=K, alphas=np.ones(K)))
            prior = StackedNormalWisharts(K, D, np.zeros((K, D)), 1e-2 * np.ones(K), np.stack(K * [np.eye(D)]), (D + 2.) * np.ones(K))
            comps = StackedGaussiansWithNormalWisharts(size=K, dim=D, prior=prior, engine=engine)
            models.append(BayesianMixtureOfGaussians(gating=gating, components=comps, engine=engine))
        return models
    return build, data


class _StartClock:
    """BatchedHipEngine that stamps the return of the start pass: a driver run is clocked from there."""

    def __init__(self, eng):
        self.eng, self.t0 = eng, None

    def random_resp_stats(self, *a, **k):
        out = self.eng.random_resp_stats(*a, **k)
        self.t0 = time.perf_counter()
        return out

    def __getattr__(self, name):
        return getattr(self.eng, name)


def run_resident_shape(sid, reps, iters=10):
    from mimo_amd.mixtures.batched import meanfield_coordinate_descent_batched
    B, N, D, K = RESIDENT_SHAPES[sid]
    solo_engine, beng = HipEngine(0), BatchedHipEngine(0)
    build, data = gmm_models(B, N, D, K, solo_engine, 300 + sid)
    kw = dict(randomize=True, init_rng='philox', seeds=list(range(B)), tol=0., sample_likelihood=False)

    def leg(resident, engine=beng):
        def run(n, out=None):
            models = build()
            clock = _StartClock(engine)
            vlbs = meanfield_coordinate_descent_batched(models, data, maxiter=n, engine=clock, resident=resident, chunk=8, **kw)
            dt = time.perf_counter() - clock.t0
            if out is not None:
                out.append(vlbs)
            return dt
        return run
    legs = {"host": leg(False), "resident": leg(True)}
    kept = {name: [] for name in legs}
    for name, fn in legs.items():                        # warm-up, and the traces that are compared
        fn(1)
        fn(1 + iters, kept[name])
    per = {name: [] for name in legs}
    for _ in range(reps):                                # the legs alternate within a repetition
        for name, fn in legs.items():
            per[name].append((fn(1 + iters) - fn(1)) / iters)
    h, r = np.array(kept["host"][0]), np.array(kept["resident"][0])
    res = {"resident_shape": sid, "B": B, "N_b": N, "Dz": D, "K": K, "iters_per_figure": iters, "reps": reps, "chunk": 8,
           "max_rel_trace_diff": float(np.max(np.abs(r - h) / np.abs(h)))}
    for name in legs:
        res[name + "_ms_per_iteration"] = float(np.median(per[name])) * 1e3
    res["speedup"] = res["host_ms_per_iteration"] / res["resident_ms_per_iteration"]
    # the host route's iteration: its passes (each returns synchronised host results) against everything else
    teng = _TimedEngine(beng)
    t0 = time.perf_counter()
    leg(False, teng)(1 + iters)
    total = time.perf_counter() - t0 - teng.upload_s
    res["host_route_pass_ms_per_iteration"] = float(np.sum(teng.pass_s)) / (1 + iters) * 1e3
    res["host_route_host_ms_per_iteration_with_start"] = (total - float(np.sum(teng.pass_s))) / (1 + iters) * 1e3
    solo_engine.close()
    beng.close()
    return res


# (B, N_b, dx, dy, K, gating): 1. the reference's parallel ILR job (examples/ilr/evaluate_sinc_parallel.py); 2., 3. shapes 2 and 3 as ILR
RESIDENT_ILR_SHAPES = {1: (24, 1600, 1, 1, 100, 'stick-breaking'), 2: (64, 10000, 1, 1, 4, 'dirichlet'),
                       3: (8, 250000, 8, 4, 64, 'stick-breaking')}


def ilr_resident_models(B, N, dx, dy, K, gating, engine, seed):
    """B mixtures of affine linear-Gaussian experts (untied blocks) on piecewise-linear data -> (build, data)."""
    from mimo_amd.distributions import (Dirichlet, CategoricalWithDirichlet, TruncatedStickBreaking, CategoricalWithStickBreaking,
                                        StackedNormalWisharts, StackedGaussiansWithNormalWisharts, StackedMatrixNormalWisharts,
                                        StackedLinearGaussiansWithMatrixNormalWisharts)
    from mimo_amd.mixtures import BayesianMixtureOfLinearGaussians
    rng = np.random.default_rng(seed)
    dc = dx + 1
    data = []
    for _ in range(B):
        centres = rng.standard_normal((K, dx)) * 4.0
        lab = rng.integers(K, size=N)
        x = centres[lab] + rng.standard_normal((N, dx))
        A = rng.standard_normal((K, dy, dc))
        y = np.einsum('nij,nj->ni', A[lab], np.hstack([x - centres[lab], np.ones((N, 1))])) + 0.1 * rng.standard_normal((N, dy))
        data.append((np.ascontiguousarray(x), np.ascontiguousarray(y)))

    def build():
        models = []
        for _ in range(B):
            if gating == 'dirichlet':
                gate = CategoricalWithDirichlet(dim=K, prior=Dirichlet(dim=K, alphas=np.ones(K)))
            else:
                gate = CategoricalWithStickBreaking(K, TruncatedStickBreaking(K, np.ones(K), 10. * np.ones(K)))
            bp = StackedNormalWisharts(K, dx, np.zeros((K, dx)), 1e-2 * np.ones(K), np.stack(K * [np.eye(dx)]), (dx + 2.) * np.ones(K))
            mp = StackedMatrixNormalWisharts(K, dc, dy, np.zeros((K, dy, dc)), np.stack(K * [1e-2 * np.eye(dc)]),
                                             np.stack(K * [np.eye(dy)]), (dy + 2.) * np.ones(K))
            models.append(BayesianMixtureOfLinearGaussians(K, dx, dy, gate, StackedGaussiansWithNormalWisharts(K, dx, bp, engine=engine),
                                                           StackedLinearGaussiansWithMatrixNormalWisharts(K, dc, dy, mp, engine=engine),
                                                           engine=engine))
        return models
    return build, data


def run_resident_ilr_shape(sid, reps, iters=10):
    """run_resident_shape for ILR models: meanfield_coordinate_descent_batched_ilr against the host route
    meanfield_coordinate_descent_batched(resident=False, sample_likelihood=False), with the spread of the repetitions."""
    from mimo_amd.mixtures.batched import meanfield_coordinate_descent_batched, meanfield_coordinate_descent_batched_ilr
    B, N, dx, dy, K, gating = RESIDENT_ILR_SHAPES[sid]
    solo_engine, beng = HipEngine(0), BatchedHipEngine(0)
    build, data = ilr_resident_models(B, N, dx, dy, K, gating, solo_engine, 400 + sid)
    kw = dict(randomize=True, init_rng='philox', seeds=list(range(B)), tol=0.)

    def leg(resident, engine=beng):
        def run(n, out=None):
            models = build()
            clock = _StartClock(engine)
            if resident:
                vlbs = meanfield_coordinate_descent_batched_ilr(models, data, maxiter=n, engine=clock, chunk=8, **kw)
            else:
                vlbs = meanfield_coordinate_descent_batched(models, data, maxiter=n, engine=clock, sample_likelihood=False, **kw)
            dt = time.perf_counter() - clock.t0
            if out is not None:
                out.append(vlbs)
            return dt
        return run
    legs = {"host": leg(False), "resident": leg(True)}
    kept = {name: [] for name in legs}
    for name, fn in legs.items():                        # warm-up, and the traces that are compared
        fn(1)
        fn(1 + iters, kept[name])
    per = {name: [] for name in legs}
    for _ in range(reps):                                # the legs alternate within a repetition
        for name, fn in legs.items():
            per[name].append((fn(1 + iters) - fn(1)) / iters)
    h, r = np.array(kept["host"][0]), np.array(kept["resident"][0])
    res = {"resident_ilr_shape": sid, "B": B, "N_b": N, "dx": dx, "dy": dy, "K": K, "gating": gating, "iters_per_figure": iters,
           "reps": reps, "chunk": 8, "max_rel_trace_diff": float(np.max(np.abs(r - h) / np.abs(h)))}
    for name in legs:
        ms = np.array(per[name]) * 1e3
        res[name + "_ms_per_iteration"] = float(np.median(ms))
        res[name + "_ms_per_iteration_min_max"] = [float(ms.min()), float(ms.max())]
        res[name + "_ms_per_iteration_all"] = [float(v) for v in ms]
    res["speedup"] = res["host_ms_per_iteration"] / res["resident_ms_per_iteration"]
    teng = _TimedEngine(beng)
    t0 = time.perf_counter()
    leg(False, teng)(1 + iters)
    total = time.perf_counter() - t0 - teng.upload_s
    res["host_route_pass_ms_per_iteration"] = float(np.sum(teng.pass_s)) / (1 + iters) * 1e3
    res["host_route_host_ms_per_iteration_with_start"] = (total - float(np.sum(teng.pass_s))) / (1 + iters) * 1e3
    solo_engine.close()
    beng.close()
    return res


class _UploadClock:
    """BatchedHipEngine that stamps the return of the upload: an SVI driver run without a random start is clocked from there."""

    def __init__(self, eng):
        self.eng, self.t0 = eng, None

    def upload(self, *a, **k):
        out = self.eng.upload(*a, **k)
        self.t0 = time.perf_counter()
        return out

    def __getattr__(self, name):
        return getattr(self.eng, name)


def run_resident_svi_shape(sid, reps, iters=10, batch=256):
    """run_resident_ilr_shape for stochastic VI: meanfield_stochastic_descent_batched(resident=True), its indices drawn on the
    host or on the device, against its host route (resident=False, sample_likelihood=False)."""
    from mimo_amd.mixtures.batched import meanfield_stochastic_descent_batched
    B, N, dx, dy, K, gating = RESIDENT_ILR_SHAPES[sid]
    N = min(N, 100000)
    solo_engine, beng = HipEngine(0), BatchedHipEngine(0)
    build, data = ilr_resident_models(B, N, dx, dy, K, gating, solo_engine, 500 + sid)
    kw = dict(randomize=False, step_size=0.5, batch_size=batch, sample_likelihood=False, numpy_seeds=list(range(B)),
              python_seeds=list(range(B)))
    routes = {"host": dict(resident=False), "resident_host_indices": dict(resident=True, chunk=8, index_rng='host'),
              "resident_philox_indices": dict(resident=True, chunk=8, index_rng='philox', seeds=list(range(B)))}

    def leg(route):
        def run(n, out=None):
            models = build()
            clock = _UploadClock(beng)
            vlbs = meanfield_stochastic_descent_batched(models, data, maxiter=n, engine=clock, **kw, **route)
            dt = time.perf_counter() - clock.t0
            if out is not None:
                out.append(vlbs)
            return dt
        return run
    legs = {name: leg(route) for name, route in routes.items()}
    kept = {name: [] for name in legs}
    for name, fn in legs.items():                        # warm-up, and the traces that are compared
        fn(1)
        fn(1 + iters, kept[name])
    per = {name: [] for name in legs}
    for _ in range(reps):                                # the legs alternate within a repetition
        for name, fn in legs.items():
            per[name].append((fn(1 + iters) - fn(1)) / iters)
    h, r = np.array(kept["host"][0]), np.array(kept["resident_host_indices"][0])
    res = {"resident_svi_shape": sid, "B": B, "N_b": N, "dx": dx, "dy": dy, "K": K, "gating": gating, "batch_size": batch,
           "iters_per_figure": iters, "reps": reps, "chunk": 8, "max_rel_trace_diff": float(np.max(np.abs(r - h) / np.abs(h)))}
    for name in legs:
        ms = np.array(per[name]) * 1e3
        res[name + "_ms_per_iteration"] = float(np.median(ms))
        res[name + "_ms_per_iteration_min_max"] = [float(ms.min()), float(ms.max())]
        res[name + "_ms_per_iteration_all"] = [float(v) for v in ms]
    for name in ("resident_host_indices", "resident_philox_indices"):
        res["speedup_" + name] = res["host_ms_per_iteration"] / res[name + "_ms_per_iteration"]
    # what the host draws of one iteration's indices cost on their own (B sample_indices calls)
    import random
    from mimo_amd.utils.data import sample_indices
    random.seed(0)
    t0 = time.perf_counter()
    for _ in range(20):
        for _ in range(B):
            sample_indices(N, batch, as_array=True)
    res["host_index_draws_ms_per_iteration"] = (time.perf_counter() - t0) / 20 * 1e3
    solo_engine.close()
    beng.close()
    return res


def resident_ilr_error_ratios():
    """One device update on every shape of tests/golden/vi_ilr_update_hp.npz: per shape and output block the largest error of the
    device and of the host route against the 50-digit values, and their ratio."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import vi_ilr_update_fixture as fx
    beng = BatchedHipEngine(0)
    out = []
    for shape in fx.shapes():
        pr = shape["prior"]
        beng.upload(shape["rows"])
        beng.weighted_stats(shape["tables"])
        beng.vi_ilr_set_prior(pr["gating"], pr["g0"], pr["g1"], pr["basis"], pr["experts"])
        beng.vi_ilr_run(shape["K"], 1, 0.)
        dev, host = fx.block_errors(beng.vi_ilr_state(shape["K"]), shape), fx.block_errors(fx.host_state(shape), shape)
        blocks = {}
        for name in fx.BLOCKS:
            d, h = float(dev[name].max()), float(host[name].max())
            blocks[name] = {"device": d, "host": h, "ratio": (d / h) if h > 0. else (1.0 if d == 0. else None)}
        out.append({"B": shape["B"], "dx": shape["dx"], "dy": shape["dy"], "K": shape["K"], "gating": shape["gating"], "blocks": blocks,
                    "worst_device": max(v["device"] for v in blocks.values()),
                    "worst_ratio": max(v["ratio"] for v in blocks.values() if v["ratio"] is not None)})
    beng.close()
    return out


def resident_error_ratios():
    """One device update on every shape of tests/golden/vi_update_hp.npz: per shape and output block the largest error of the
    device and of the host-native route against the 50-digit values, and their ratio."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import vi_update_fixture as fx
    beng = BatchedHipEngine(0)
    out = []
    for shape in fx.shapes():
        beng.upload(shape["rows"])
        beng.weighted_stats(shape["tables"])
        beng.vi_set_prior(**shape["prior"])
        beng.vi_run(shape["K"], 1, 0.)
        dev, host = fx.block_errors(beng.vi_state(shape["K"]), shape), fx.block_errors(fx.host_state(shape), shape)
        blocks = {}
        for name in fx.BLOCKS:
            d, h = float(dev[name].max()), float(host[name].max())
            blocks[name] = {"device": d, "host": h, "ratio": (d / h) if h > 0. else (1.0 if d == 0. else None)}
        out.append({"B": shape["B"], "Dz": shape["D"], "K": shape["K"], "blocks": blocks,
                    "worst_ratio": max(v["ratio"] for v in blocks.values() if v["ratio"] is not None)})
    beng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="1,2,3")
    ap.add_argument("--no-driver", action="store_true", help="skip the driver timings (VI iteration, Gibbs sweep)")
    ap.add_argument("--no-gibbs", action="store_true", help="skip the Gibbs leg")
    ap.add_argument("--no-start", action="store_true", help="skip the start leg")
    ap.add_argument("--start-only", action="store_true", help="only the start leg")
    ap.add_argument("--trace-start", type=int, default=0, metavar="SHAPE", help="only run the batched start passes of SHAPE")
    ap.add_argument("--svi", action="store_true", help="only the SVI leg (selection pass, SVI iteration)")
    ap.add_argument("--trace-svi", type=int, default=0, metavar="SHAPE", help="only run the selection pass and the plain pass of SHAPE")
    ap.add_argument("--predict", action="store_true", help="only the prediction leg (batched predict against B solo predicts)")
    ap.add_argument("--trace-predict", type=int, default=0, metavar="SHAPE", help="only run the batched and the solo predictions of SHAPE")
    ap.add_argument("--nested", action="store_true", help="only the nested leg (nested VI driver against the solo mixture of mixtures)")
    ap.add_argument("--resident", action="store_true", help="only the resident leg (device-resident VI loop against the host route)")
    ap.add_argument("--resident-ilr", action="store_true",
                    help="only the resident ILR leg (device-resident loop for mixtures of linear-Gaussian experts against the host route)")
    ap.add_argument("--resident-svi", action="store_true",
                    help="only the resident SVI leg (device-resident SVI loop, host and device index draws, against the host route)")
    args = ap.parse_args()
    if args.resident_svi:
        os.makedirs(args.out, exist_ok=True)
        res = {"timings": []}
        path = os.path.join(args.out, "batched_resident_svi.json")
        for s in args.shapes.split(","):
            if int(s) in RESIDENT_ILR_SHAPES:
                res["timings"].append(run_resident_svi_shape(int(s), args.reps))
                print(json.dumps({k: v for k, v in res["timings"][-1].items() if not k.endswith("_all")}), flush=True)
                with open(path, "w") as f:               # (after every shape: a long run leaves what it has)
                    json.dump(res, f, indent=1)
        return
    if args.resident_ilr:
        os.makedirs(args.out, exist_ok=True)
        res = {"timings": [], "update_error_vs_50_digits": resident_ilr_error_ratios()}
        print(json.dumps([{k: e[k] for k in ("dx", "dy", "K", "worst_device", "worst_ratio")} for e in res["update_error_vs_50_digits"]]))
        path = os.path.join(args.out, "batched_resident_ilr_vi.json")
        for s in args.shapes.split(","):
            if int(s) in RESIDENT_ILR_SHAPES:
                res["timings"].append(run_resident_ilr_shape(int(s), args.reps))
                print(json.dumps({k: v for k, v in res["timings"][-1].items() if not k.endswith("_all")}), flush=True)
                with open(path, "w") as f:               # (after every shape: a long run leaves what it has)
                    json.dump(res, f, indent=1)
        return
    if args.resident:
        os.makedirs(args.out, exist_ok=True)
        res = {"timings": [run_resident_shape(int(s), args.reps) for s in args.shapes.split(",") if int(s) in RESIDENT_SHAPES],
               "update_error_vs_50_digits": resident_error_ratios()}
        for r in res["timings"]:
            print(json.dumps(r))
        print(json.dumps([{k: e[k] for k in ("B", "Dz", "K", "worst_ratio")} for e in res["update_error_vs_50_digits"]]))
        with open(os.path.join(args.out, "batched_resident_vi.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    if args.nested:
        os.makedirs(args.out, exist_ok=True)
        res = [run_nested_shape(int(s), args.reps) for s in args.shapes.split(",") if int(s) in NESTED_SHAPES]
        for r in res:
            print(json.dumps(r))
        with open(os.path.join(args.out, "bench_batched_nested.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    if args.trace_predict:
        trace_predict(args.trace_predict)
        return
    if args.predict:
        os.makedirs(args.out, exist_ok=True)
        res = [run_predict_shape(int(s), args.reps) for s in args.shapes.split(",")]
        for r in res:
            print(json.dumps(r))
        with open(os.path.join(args.out, "bench_batched_predict.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    if args.trace_svi:
        trace_svi(args.trace_svi)
        return
    if args.svi:
        os.makedirs(args.out, exist_ok=True)
        res = [run_svi_shape(int(s), args.reps) for s in args.shapes.split(",")]
        if not args.no_driver:
            res.append(svi_driver_iteration(args.reps))
        for r in res:
            print(json.dumps(r))
        with open(os.path.join(args.out, "bench_batched_svi.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    if args.trace_start:
        trace_start(args.trace_start)
        return
    os.makedirs(args.out, exist_ok=True)
    if args.start_only:
        res = [run_start_shape(int(s), args.reps) for s in args.shapes.split(",")]
        for r in res:
            print(json.dumps(r))
        with open(os.path.join(args.out, "bench_batched_start.json"), "w") as f:
            json.dump(res, f, indent=1)
        return
    res = [run_shape(int(s), args.reps) for s in args.shapes.split(",")]
    if not args.no_start:
        res += [run_start_shape(int(s), args.reps) for s in args.shapes.split(",")]
    if not args.no_driver:
        res.append(driver_iteration(min(args.reps, 10)))
    if not args.no_gibbs:
        res += [run_gibbs_shape(int(s), args.reps) for s in args.shapes.split(",")]
        if not args.no_driver:
            res.append(gibbs_driver_sweep(args.reps))
    for r in res:
        print(json.dumps(r))
    with open(os.path.join(args.out, "bench_batched.json"), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
