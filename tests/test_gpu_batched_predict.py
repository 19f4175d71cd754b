"""GPU: batched prediction (mimo_predict_batched / BatchedHipEngine.predict / meanfield_prediction_batched).

Contract: (1) problem b's outputs are np.array_equal to the solo HipEngine.predict on the uploaded rows
(X_b - shift_b) / scale_b computed with NumPy; (2) they are the same bits alone, at any position of any batch, in the shared
form as in the ragged form; (3) they match oracle.mimo_oracle.predict_canonical within the solo kernel's tolerances
(mu 1e-11, covar 1e-10, nlpd 1e-11 relative: tests/test_gpu_parity.py); (4) the driver equals each model's solo
meanfield_prediction bit for bit and reproduces the reference's prediction fixtures at 1e-6; (5) nothing resident changes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import numpy.random as npr
import pytest

from conftest import load_golden, rel_err
import model_checks as mc
from oracle import mimo_oracle as O
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.engine import HipEngine
from mimo_amd.mixtures.batched import meanfield_prediction_batched
from mimo_amd.mixtures.ilr import Standardizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("c", "b", "W", "M", "Q", "Cc")


@pytest.fixture(scope="module")
def beng():
    eng = BatchedHipEngine(0)
    yield eng
    eng.close()


def _params(rng, B, K, dx, dy):
    """B problems' gate (c, b, W) and predictive blocks (M, Q, Cc, P, ld), as test_predict_kernel_vs_oracle draws them."""
    dc = dx + 1

    def spd(d, ridge):
        A = rng.standard_normal((B, K, d, d))
        return A @ np.swapaxes(A, -1, -2) / d + ridge * np.eye(d)
    W = spd(dx, 0.3)
    m = rng.standard_normal((B, K, dx)) * 2
    b = np.einsum('pkde,pke->pkd', W, m)
    c = -0.5 * np.einsum('pkd,pkd->pk', m, b) + rng.standard_normal((B, K)) * 0.1
    P = spd(dy, 0.5)
    return dict(c=c, b=b, W=W, M=rng.standard_normal((B, K, dy, dc)), Q=spd(dc, 0.1), Cc=np.linalg.inv(P), P=P,
                ld=np.linalg.slogdet(P)[1])


def _rows(rng, counts, dx, dy, constant_column=True):
    """Per problem raw rows (well away from standardised), targets and the (shift, scale) blocks of a Standardizer fitted on
    them; column 0 of problem 0 is constant (zero variance: scale 1, shift nonzero)."""
    xs = [rng.standard_normal((n, dx)) * 3. + 5. for n in counts]
    ys = [rng.standard_normal((n, dy)) * 2. - 1. for n in counts]
    if constant_column and counts[0] > 0:
        xs[0][:, 0] = 2.5
    x_tf, y_tf = [], []
    for x, y in zip(xs, ys):
        for a, out, d in ((x, x_tf, dx), (y, y_tf, dy)):
            if len(a):
                t = Standardizer().fit(a)
                out.append(np.stack([t.mean_, t.scale_]))
            else:
                out.append(np.stack([np.zeros(d), np.ones(d)]))
    return xs, ys, np.stack(x_tf), np.stack(y_tf)


def _call(eng, x, par, y=None, idx=None, **kw):
    """BatchedHipEngine.predict on the problems idx (default all) of par."""
    sel = (lambda a: a) if idx is None else (lambda a: a[np.asarray(idx)])
    extra = dict(P=sel(par["P"]), ld=sel(par["ld"])) if y is not None else {}
    for k in ("x_transform", "y_transform"):
        if kw.get(k) is not None:
            kw[k] = sel(kw[k])
    return eng.predict(x, *(sel(par[k]) for k in NAMES), y=y, **extra, **kw)


def _solo(engine, x, par, i, x_tf=None, y=None, y_tf=None, mode='average', variance='full'):
    """HipEngine.predict of problem i on the rows standardised with NumPy."""
    xt = np.ascontiguousarray((x - x_tf[i, 0]) / x_tf[i, 1] if x_tf is not None else x)
    yt = None if y is None else np.ascontiguousarray((y - y_tf[i, 0]) / y_tf[i, 1] if y_tf is not None else y)
    engine.upload(xt)
    res = engine.predict(*(par[k][i] for k in NAMES), mode=mode, y=yt, P=par["P"][i] if y is not None else None,
                         ld=par["ld"][i] if y is not None else None, variance=variance)
    return res, xt, yt


def _flat(r):
    mu, second, nlpd = r
    return [mu] + (list(second) if isinstance(second, tuple) else [second]) + ([] if nlpd is None else [nlpd])


def _same(a, b):
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb)
    for u, v in zip(fa, fb):
        assert u.shape == v.shape and np.array_equal(u, v)


@pytest.mark.parametrize("dx", range(1, 9))
def test_every_instantiation_equals_solo_and_the_oracle(engine, beng, dx):
    counts, K = (257, 1, 0), 5
    for dy in range(1, 9):
        rng = np.random.default_rng(100 * dx + dy)
        par = _params(rng, 3, K, dx, dy)
        xs, ys, x_tf, y_tf = _rows(rng, counts, dx, dy)
        for mode in ("average", "mode"):
            full = _call(beng, xs, par, y=ys, mode=mode, x_transform=x_tf, y_transform=y_tf)
            diag = _call(beng, xs, par, y=ys, mode=mode, variance='diagonal', x_transform=x_tf, y_transform=y_tf)
            for i, n in enumerate(counts):
                mu, covar, nlpd = full[i]
                assert mu.shape == (n, dy) and covar.shape == (n, dy, dy) and nlpd.shape == (n,)
                assert diag[i][1][0].shape == (n, dy) and diag[i][1][1].shape == (n, dy)
                if n == 0:
                    continue
                ref, xt, yt = _solo(engine, xs[i], par, i, x_tf, ys[i], y_tf, mode)
                _same(full[i], ref)
                _same(diag[i], engine.predict(*(par[k][i] for k in NAMES), mode=mode, y=yt, P=par["P"][i], ld=par["ld"][i],
                                              variance='diagonal'))
                rmu, rcov, rnl = O.predict_canonical(xt, *(par[k][i] for k in NAMES), True, mode, yt, par["P"][i], par["ld"][i])
                assert rel_err(mu, rmu) < 1e-11 and rel_err(covar, rcov) < 1e-10 and rel_err(nlpd, rnl) < 1e-11, (dy, mode, i)


def test_row_counts_alone_and_permuted(engine, beng):
    counts, K, dx, dy = (0, 1, 255, 256, 257, 512, 513, 1000), 7, 2, 2
    rng = np.random.default_rng(7)
    par = _params(rng, len(counts), K, dx, dy)
    xs, ys, x_tf, y_tf = _rows(rng, counts, dx, dy, constant_column=False)
    perm = [5, 0, 7, 2, 1, 6, 4, 3]
    for mode in ("average", "mode"):
        kw = dict(mode=mode, x_transform=x_tf, y_transform=y_tf)
        res = _call(beng, xs, par, y=ys, **kw)
        permuted = _call(beng, [xs[i] for i in perm], par, y=[ys[i] for i in perm], idx=perm, **dict(kw))
        for j, i in enumerate(perm):
            _same(permuted[j], res[i])
        for i, n in enumerate(counts):
            alone, = _call(beng, [xs[i]], par, y=[ys[i]], idx=[i], **dict(kw))
            _same(alone, res[i])
            if n:
                _same(res[i], _solo(engine, xs[i], par, i, x_tf, ys[i], y_tf, mode)[0])


def test_all_empty_and_single_problem_batches(engine, beng):
    rng = np.random.default_rng(8)
    dx, dy, K = 3, 2, 4
    par = _params(rng, 2, K, dx, dy)
    for res in (_call(beng, [np.zeros((0, dx))] * 2, par), _call(beng, np.zeros((0, dx)), par),
                _call(beng, [np.zeros((0, dx))] * 2, par, y=[np.zeros((0, dy))] * 2, variance='diagonal')):
        assert len(res) == 2 and all(r[0].shape == (0, dy) for r in res)
    x = rng.standard_normal((300, dx))
    one, = _call(beng, x, par, idx=[1])
    _same(one, _solo(engine, x, par, 1)[0])
    one, = _call(beng, [x], par, idx=[1])
    _same(one, _solo(engine, x, par, 1)[0])


@pytest.mark.parametrize("N", [1, 256, 300])
def test_shared_form_equals_ragged_and_solo(engine, beng, N):
    rng = np.random.default_rng(N)
    B, dx, dy, K = 5, 3, 2, 6
    par = _params(rng, B, K, dx, dy)
    x, y = rng.standard_normal((N, dx)) * 2. + 1., rng.standard_normal((N, dy))
    _, _, x_tf, y_tf = _rows(rng, [40] * B, dx, dy, constant_column=False)
    for mode, variance in (("average", "full"), ("mode", "diagonal")):
        kw = dict(mode=mode, variance=variance, x_transform=x_tf, y_transform=y_tf)
        shared = _call(beng, x, par, y=y, **kw)
        ragged = _call(beng, [x] * B, par, y=[y] * B, **dict(kw))
        for i in range(B):
            _same(shared[i], ragged[i])
            _same(shared[i], _solo(engine, x, par, i, x_tf, y, y_tf, mode, variance)[0])


@pytest.mark.parametrize("dx,dy", [(1, 1), (8, 4)])
def test_component_counts(engine, beng, dx, dy):
    for K in (1, 16, 100, 130):
        rng = np.random.default_rng(K + dx)
        par = _params(rng, 2, K, dx, dy)
        xs, ys, x_tf, y_tf = _rows(rng, (300, 70), dx, dy)
        for mode in ("average", "mode"):
            res = _call(beng, xs, par, y=ys, mode=mode, x_transform=x_tf, y_transform=y_tf)
            for i in range(2):
                ref, xt, yt = _solo(engine, xs[i], par, i, x_tf, ys[i], y_tf, mode)
                _same(res[i], ref)
                rmu, rcov, rnl = O.predict_canonical(xt, *(par[k][i] for k in NAMES), True, mode, yt, par["P"][i], par["ld"][i])
                assert rel_err(res[i][0], rmu) < 1e-11 and rel_err(res[i][1], rcov) < 1e-10 and rel_err(res[i][2], rnl) < 1e-11


def test_extremes(engine, beng):
    rng = np.random.default_rng(11)
    B, dx, dy, K = 2, 2, 2, 5
    par = _params(rng, B, K, dx, dy)
    par["c"][:, 2] = -1e300                                   # a switched-off component
    xs = [rng.standard_normal((300, dx)), rng.standard_normal((300, dx)) * 1e3 + 1e3]     # rows 1e3 deviations from every gate
    ys = [rng.standard_normal((300, dy)) for _ in range(B)]
    for mode in ("average", "mode"):
        res = _call(beng, xs, par, y=ys, mode=mode)
        for i in range(B):
            assert all(np.all(np.isfinite(a)) for a in _flat(res[i]))
            _same(res[i], _solo(engine, xs[i], par, i, y=ys[i], mode=mode)[0])


def test_no_transforms_equal_the_identity_transform(beng):
    rng = np.random.default_rng(12)
    B, dx, dy, K = 3, 4, 3, 6
    par = _params(rng, B, K, dx, dy)
    xs, ys, _, _ = _rows(rng, (100, 257, 3), dx, dy)
    ident = lambda d: np.stack([np.stack([np.zeros(d), np.ones(d)])] * B)
    for variance in ("full", "diagonal"):
        plain = _call(beng, xs, par, y=ys, variance=variance)
        unit = _call(beng, xs, par, y=ys, variance=variance, x_transform=ident(dx), y_transform=ident(dy))
        for a, b in zip(plain, unit):
            _same(a, b)


def _raw(eng, B, x, row_off, N_shared, dx, par, dy, flags=0, mode=0):
    """mimo_predict_batched through ctypes: -> (return code, error text)."""
    K = par["c"].shape[1]
    n = max(int(row_off[-1]) if row_off is not None else N_shared * B, 1)
    mu, cov = np.empty(n * dy), np.empty(n * dy * max(dy, 2))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = eng._lib.mimo_predict_batched(eng._ctx, B, p(x), p(row_off), N_shared, dx, None, p(par["c"]), p(par["b"]), p(par["W"]), K,
                                       p(par["M"]), p(par["Q"]), p(par["Cc"]), dy, mode, None, None, None, None, p(mu), p(cov),
                                       None, flags)
    return rc, eng._lib.mimo_last_error(eng._ctx).decode()


def test_refusals(beng):
    rng = np.random.default_rng(13)
    B, K = 2, 3
    off = np.array([0, 4, 6], dtype=np.int64)
    par9x, par9y, par = _params(rng, B, K, 9, 2), _params(rng, B, K, 2, 9), _params(rng, B, K, 2, 2)
    rc, msg = _raw(beng, B, np.zeros((6, 9)), off, 0, 9, par9x, 2)
    assert rc == _lib.E_UNSUPPORTED and "dx <= 8" in msg
    rc, msg = _raw(beng, B, np.zeros((6, 2)), off, 0, 2, par9y, 9)
    assert rc == _lib.E_UNSUPPORTED and "dy <= 8" in msg
    x = np.zeros((6, 2))
    rc, msg = _raw(beng, B, x, off, 0, 2, par, 2, flags=_lib.F_DEVICE_OUT)
    assert rc == _lib.E_INVALID and "MIMO_F_DIAG_VAR" in msg
    rc, msg = _raw(beng, B, x, np.array([0, 4, 3], dtype=np.int64), 0, 2, par, 2)
    assert rc == _lib.E_INVALID and "row_off decreases" in msg
    rc, msg = _raw(beng, B, x, np.array([1, 4, 6], dtype=np.int64), 0, 2, par, 2)
    assert rc == _lib.E_INVALID and "row_off[0]" in msg
    rc, msg = _raw(beng, B, x, off, 6, 2, par, 2)
    assert rc == _lib.E_INVALID and "N_shared" in msg
    rc, msg = _raw(beng, B, x, None, -1, 2, par, 2)
    assert rc == _lib.E_INVALID and "N_shared" in msg
    rc, msg = _raw(beng, B, x, off, 0, 2, par, 2, mode=2)
    assert rc == _lib.E_INVALID and "mode" in msg
    assert _raw(beng, B, x, off, 0, 2, par, 2)[0] == 0
    # through Python: the library's refusal arrives as MimoHipError with the bound in its text
    with pytest.raises(_lib.MimoHipError, match="dx <= 8"):
        _call(beng, np.zeros((6, 9)), par9x)
    with pytest.raises(_lib.MimoHipError, match="dy <= 8"):
        _call(beng, np.zeros((6, 2)), par9y)


def test_nothing_resident_changes(beng):
    rng = np.random.default_rng(14)
    eng = BatchedHipEngine(0)
    try:
        B, D, K = 3, 3, 5
        Zs = [rng.standard_normal((n, D)) for n in (300, 33, 1000)]
        A = rng.standard_normal((B, K, D, D))
        c, b, W = rng.standard_normal((B, K)), rng.standard_normal((B, K, D)), A @ A.transpose(0, 1, 3, 2) / D + 0.3 * np.eye(D)
        eng.upload(Zs)
        par = _params(rng, 4, 9, 2, 3)
        xs, ys, x_tf, y_tf = _rows(rng, (700, 5, 0, 258), 2, 3)
        kw = dict(x_transform=x_tf, y_transform=y_tf, variance='diagonal')
        fresh = _call(beng, xs, par, y=ys, **dict(kw))

        S0, sc0 = eng.estep(c, b, W, keep_lse=True)
        lse0 = eng.get_lse()
        for a, r in zip(_call(eng, xs, par, y=ys, **dict(kw)), fresh):
            _same(a, r)
        for u, v in zip(eng.get_lse(), lse0):
            assert np.array_equal(u, v)
        labels0, L0 = eng.gibbs_labels(c, b, W, seeds=[1, 2, 3], sweep=4)
        for a, r in zip(_call(eng, xs, par, y=ys, **dict(kw)), fresh):
            _same(a, r)
        for u, v in zip(eng.get_labels(), labels0):
            assert np.array_equal(u, v)
        S1, sc1 = eng.estep(c, b, W, keep_lse=True)
        assert np.array_equal(sc1, sc0) and all(np.array_equal(u.packed(), v.packed()) for u, v in zip(S1, S0))
        assert (eng.B, eng.D) == (3, 3) and np.array_equal(eng.row_off, [0, 300, 333, 1333])
    finally:
        eng.close()


def test_fresh_engine_and_one_engine_across_shapes():
    rng = np.random.default_rng(15)
    shapes = [(3, 4, 1, 1, (300, 0, 17)), (2, 70, 8, 4, (1000, 257)), (5, 3, 2, 8, (1, 2, 3, 4, 600))]
    cases = []
    for B, K, dx, dy, counts in shapes:
        par = _params(rng, B, K, dx, dy)
        cases.append((par,) + _rows(rng, counts, dx, dy))
    reused = BatchedHipEngine(0)
    try:
        for par, xs, ys, x_tf, y_tf in cases:
            fresh = BatchedHipEngine(0)                        # nothing uploaded, first call of its context
            try:
                want = _call(fresh, xs, par, y=ys, x_transform=x_tf, y_transform=y_tf)
            finally:
                fresh.close()
            for a, r in zip(_call(reused, xs, par, y=ys, x_transform=x_tf, y_transform=y_tf), want):
                _same(a, r)
    finally:
        reused.close()


def _capture_fitted_tied(name, engine, monkeypatch):
    got = []
    monkeypatch.setattr(mc, "check_prediction", lambda ilr, g, tol: got.append((ilr, g)))
    mc.check_tied_ilr_prediction(name, engine)
    monkeypatch.undo()
    return got[0]


def test_driver_equals_solo(engine, beng, monkeypatch):
    g = load_golden("ilr_dx1_dy1_k6_dir")
    X, Y = g["X"], g["Y"]
    rng = np.random.default_rng(16)
    models = []
    for i in range(4):
        idx = rng.permutation(len(X))[:240]
        kind, ilr = mc.build_ilr(g, engine)
        ilr.init_transform(X[idx], Y[idx])
        if i == 3:
            ilr.scale = False
        npr.seed(60 + i)
        ilr.meanfield_coordinate_descent(X[idx], Y[idx], randomize=True, maxiter=5, progress_bar=False)
        models.append(ilr)
    xq = np.linspace(-12., 12., 300).reshape(-1, 1)
    yq = np.sinc(xq / np.pi)
    rx, ry = [xq, xq[:1], xq[:0], xq[10:270]], [yq, yq[:1], yq[:0], yq[10:270]]
    combos = [(p, v, inc, wy) for p in ("average", "mode") for v in ("diagonal", "full") for inc in (False, True)
              for wy in (False, True)]
    solo = {cb: ([m.meanfield_prediction(xq, yq if cb[3] else None, prediction=cb[0], variance=cb[1], incremental=cb[2])
                  for m in models],
                 [m.meanfield_prediction(xi, yi if cb[3] else None, prediction=cb[0], variance=cb[1], incremental=cb[2])
                  for m, xi, yi in zip(models, rx, ry) if len(xi)]) for cb in combos}

    def refuse(*a, **k):
        raise AssertionError("the batched prediction must not touch the solo engine")
    monkeypatch.setattr(HipEngine, "predict", refuse)
    monkeypatch.setattr(HipEngine, "upload", refuse)
    for cb in combos:
        kw = dict(prediction=cb[0], variance=cb[1], incremental=cb[2], engine=beng)
        shared = meanfield_prediction_batched(models, xq, yq if cb[3] else None, **kw)
        ragged = meanfield_prediction_batched(models, rx, ry if cb[3] else None, **kw)
        for r, s in zip(shared, solo[cb][0]):
            assert len(r) == len(s) and all(np.array_equal(u, v) for u, v in zip(r, s)), cb
        for r, s in zip([r for r, xi in zip(ragged, rx) if len(xi)], solo[cb][1]):
            assert len(r) == len(s) and all(np.array_equal(u, v) for u, v in zip(r, s)), cb
        assert ragged[2][0].shape == (0, 1)


@pytest.mark.parametrize("name", ["tied_ilr_sine_k8", "tied_ilr_dx3_dy2_k6"])
def test_driver_reproduces_the_reference_fixtures(engine, beng, monkeypatch, name):
    ilr, g = _capture_fitted_tied(name, engine, monkeypatch)
    X, tol = g["X"], 1e-6
    for pred in ("average", "mode"):
        (mu, var, std), = meanfield_prediction_batched([ilr], X, prediction=pred, engine=beng)
        assert rel_err(mu, g[f"pred_{pred}_gaussian_mu"]) < tol, pred
        assert rel_err(var, g[f"pred_{pred}_gaussian_var"]) < tol, pred
        assert rel_err(std, g[f"pred_{pred}_gaussian_std"]) < tol, pred
    (mu, covar, std), = meanfield_prediction_batched([ilr], X, prediction='average', variance='full', engine=beng)
    assert rel_err(covar, g["pred_average_gaussian_covar"]) < tol


def test_example_prints_the_ensemble_summary():
    cmd = [sys.executable, os.path.join(ROOT, "examples", "ilr_sinc_batched.py"), "--fits", "3", "--rows", "400", "--experts", "10",
           "--iters", "5", "--predict"]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    line = [ln for ln in proc.stdout.splitlines() if "RMSE of the ensemble mean" in ln]
    assert len(line) == 1 and "3 models on 400 inputs" in line[0] and "mean ensemble spread" in line[0]
