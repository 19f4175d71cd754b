"""CPU: batched prediction without a GPU — the new entry point fails loudly on a null context, the argument validation of
BatchedHipEngine.predict happens before any library call, meanfield_prediction_batched on a duck-typed batched engine
backed by the CPU oracle reproduces the reference's tied-ILR prediction fixtures (B = 1) and the solo meanfield_prediction
of three differently seeded fits (B = 3) in every option combination, the solo method is unchanged by the shared host
tail, and the new kernel file's ISA passes the barrier check."""
import os
import subprocess
import sys

import numpy as np
import numpy.random as npr
import pytest

from conftest import load_golden, rel_err
import model_checks as mc
from oracle_engine import OracleEngine
from oracle import mimo_oracle as O
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.mixtures.batched import meanfield_prediction_batched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_entry_point_fails_loudly_on_a_null_context():
    lib = _lib.load()
    one = np.ones((1, 1, 1, 1))
    p = one.ctypes.data
    out = np.empty(4)
    assert lib.mimo_predict_batched(None, 1, p, None, 1, 1, None, p, p, p, 1, p, p, p, 1, 0, None, None, None, None,
                                    out.ctypes.data, out.ctypes.data, None, 0) == _lib.E_INVALID
    assert lib.mimo_predict_batched(None, 1, None, None, 0, 1, None, None, None, None, 1, None, None, None, 1, 0, None, None,
                                    None, None, None, None, None, 0) == _lib.E_INVALID


def _offline():
    """An engine object without a context or a library: only the host-side validation runs."""
    eng = object.__new__(BatchedHipEngine)
    eng._ctx, eng.B, eng.D = None, 7, 5                   # (predict reads neither B nor D)
    eng.row_off = np.zeros(1, dtype=np.int64)
    return eng


def _blocks(B=3, K=4, dx=2, dy=3):
    return dict(c=np.zeros((B, K)), b=np.zeros((B, K, dx)), W=np.zeros((B, K, dx, dx)), M=np.zeros((B, K, dy, dx + 1)),
                Q=np.zeros((B, K, dx + 1, dx + 1)), Cc=np.zeros((B, K, dy, dy)))


def test_predict_argument_validation():
    eng = _offline()
    B, K, dx, dy = 3, 4, 2, 3
    good = _blocks(B, K, dx, dy)
    xs, ys = np.zeros((5, dx)), np.zeros((5, dy))
    xr, yr = [np.zeros((5, dx)), np.zeros((1, dx)), np.zeros((0, dx))], [np.zeros((5, dy)), np.zeros((1, dy)), np.zeros((0, dy))]
    P, ld = np.zeros((B, K, dy, dy)), np.zeros((B, K))
    tf = lambda d, scale=1.: np.stack([np.stack([np.zeros(d), np.full(d, scale)])] * B)

    def call(x=xs, **kw):
        args = dict(good)
        extra = {k: kw.pop(k) for k in list(kw) if k not in args}
        args.update(kw)
        return eng.predict(x, args["c"], args["b"], args["W"], args["M"], args["Q"], args["Cc"], **extra)

    # a wrong leading B in any block
    for name in ("b", "W", "M", "Q", "Cc"):
        with pytest.raises(ValueError):
            call(**{name: good[name][:2]})
    with pytest.raises(ValueError):
        call(c=np.zeros(K))
    with pytest.raises(ValueError):
        call(y=ys, P=P[:2], ld=ld)
    with pytest.raises(ValueError):
        call(y=ys, P=P, ld=ld[:2])
    # dc != dx + 1 (no affine column, or one too many)
    with pytest.raises(ValueError):
        call(M=np.zeros((B, K, dy, dx)), Q=np.zeros((B, K, dx, dx)))
    with pytest.raises(ValueError):
        call(M=np.zeros((B, K, dy, dx + 2)), Q=np.zeros((B, K, dx + 2, dx + 2)))
    # rows: wrong width, wrong count of problems, x and y in mixed forms, y rows that do not match x
    with pytest.raises(ValueError):
        call(x=np.zeros((5, dx + 1)))
    with pytest.raises(ValueError):
        call(x=xr[:2])
    with pytest.raises(ValueError):
        call(x=xs, y=yr, P=P, ld=ld)
    with pytest.raises(ValueError):
        call(x=xr, y=ys, P=P, ld=ld)
    with pytest.raises(ValueError):
        call(x=xr, y=yr[::-1], P=P, ld=ld)
    # y without P / ld
    with pytest.raises(ValueError):
        call(y=ys)
    with pytest.raises(ValueError):
        call(y=ys, P=P)
    with pytest.raises(ValueError):
        call(y=ys, ld=ld)
    # transform blocks: wrong shape, zero or non-finite scale, y_transform without y
    for bad in (tf(dx)[:2], tf(dx + 1), tf(dx)[:, :1], tf(dx, 0.), tf(dx, np.inf), tf(dx, np.nan)):
        with pytest.raises(ValueError):
            call(x_transform=bad)
    for bad in (tf(dx), tf(dy, 0.)):
        with pytest.raises(ValueError):
            call(y=ys, P=P, ld=ld, y_transform=bad)
    with pytest.raises(ValueError):
        call(y_transform=tf(dy))
    # variance and mode outside the allowed values
    with pytest.raises(ValueError):
        call(variance='diag')
    with pytest.raises(ValueError):
        call(mode='max')
    # well-formed arguments pass the validation (and then need the library: the offline object has none)
    for kw in (dict(), dict(x=xr), dict(y=ys, P=P, ld=ld, y_transform=tf(dy, 2.)), dict(x=xr, y=yr, P=P, ld=ld, mode='mode'),
               dict(x_transform=tf(dx, -0.5), variance='diagonal')):
        with pytest.raises(AttributeError):
            call(**kw)


class OracleBatchPredict:
    """Duck-typed batched engine on the CPU oracle: predict() with BatchedHipEngine's signature — predict_canonical on each
    problem's rows (x_b - shift_b) / scale_b."""
    device = 0

    def __init__(self):
        self.calls = 0

    def predict(self, x, c, b, W, M, Q, Cc, mode='average', y=None, P=None, ld=None, variance='full', x_transform=None,
                y_transform=None):
        self.calls += 1
        out = []
        for i in range(c.shape[0]):
            xi = np.asarray(x[i] if isinstance(x, list) else x, float)
            if x_transform is not None:
                xi = (xi - x_transform[i, 0]) / x_transform[i, 1]
            yi = None
            if y is not None:
                yi = np.asarray(y[i] if isinstance(y, list) else y, float)
                if y_transform is not None:
                    yi = (yi - y_transform[i, 0]) / y_transform[i, 1]
            mu, covar, nlpd = O.predict_canonical(xi, c[i], b[i], W[i], M[i], Q[i], Cc[i], True, mode, yi,
                                                  None if y is None else P[i], None if y is None else ld[i])
            if variance == 'diagonal':
                var = np.diagonal(covar, axis1=1, axis2=2).copy()
                covar = (var, np.sqrt(var))
            out.append((mu, covar, nlpd))
        return out


@pytest.fixture(scope="module", params=["tied_ilr_sine_k8", "tied_ilr_dx3_dy2_k6"])
def fitted_tied(request):
    """The fixture's tied-ILR model as check_tied_ilr_prediction fits it on the CPU oracle, taken where that check hands
    it to check_prediction."""
    got = []
    orig = mc.check_prediction
    mc.check_prediction = lambda ilr, g, tol: got.append((ilr, g))
    try:
        mc.check_tied_ilr_prediction(request.param, OracleEngine())
    finally:
        mc.check_prediction = orig
    return got[0]


def test_solo_prediction_is_unchanged_by_the_shared_tail(fitted_tied):
    ilr, g = fitted_tied
    mc.check_prediction(ilr, g, tol=1e-6)


def test_one_tied_model_reproduces_the_reference_prediction(fitted_tied):
    ilr, g = fitted_tied
    X, tol = g["X"], 1e-6
    eng = OracleBatchPredict()
    for pred in ("average", "mode"):
        (mu, var, std), = meanfield_prediction_batched([ilr], X, prediction=pred, engine=eng)
        assert rel_err(mu, g[f"pred_{pred}_gaussian_mu"]) < tol, pred
        assert rel_err(var, g[f"pred_{pred}_gaussian_var"]) < tol, pred
        assert rel_err(std, g[f"pred_{pred}_gaussian_std"]) < tol, pred
    (mu, covar, std), = meanfield_prediction_batched([ilr], X, prediction='average', variance='full', engine=eng)
    assert rel_err(covar, g["pred_average_gaussian_covar"]) < tol
    assert eng.calls == 3


def _same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.shape == v.shape and np.array_equal(u, v)


def _short_fits(scales=(True, True, False)):
    """Three stacked ILR models of one shape, differently seeded short fits on the CPU oracle."""
    g = load_golden("ilr_svi_dx2_dy1_k8")
    X, Y = g["X"], g["Y"]
    rng = np.random.default_rng(12)
    models = []
    for i, scale in enumerate(scales):
        idx = rng.permutation(len(X))[:200 + 20 * i]
        kind, ilr = mc.build_ilr(g, OracleEngine())
        ilr.init_transform(X[idx], Y[idx])
        ilr.scale = scale                                   # (False: the model works on the raw rows)
        npr.seed(50 + i)
        ilr.meanfield_coordinate_descent(X[idx], Y[idx], randomize=True, maxiter=3, progress_bar=False)
        models.append(ilr)
    return models, X, Y


def test_three_models_equal_their_solo_predictions():
    models, X, Y = _short_fits()
    xq, yq = X[:37] * 1.1, Y[:37]
    ragged_x = [xq, X[40:41], X[:0]]
    ragged_y = [yq, Y[40:41], Y[:0]]
    eng = OracleBatchPredict()
    for pred in ("average", "mode"):
        for variance in ("diagonal", "full"):
            for incremental in (False, True):
                kw = dict(prediction=pred, variance=variance, incremental=incremental)
                for with_y in (False, True):
                    res = meanfield_prediction_batched(models, xq, yq if with_y else None, engine=eng, **kw)
                    for m, r in zip(models, res):
                        _same(r, m.meanfield_prediction(xq, yq if with_y else None, **kw))
                    res = meanfield_prediction_batched(models, ragged_x, ragged_y if with_y else None, engine=eng, **kw)
                    for m, r, xi, yi in zip(models, res, ragged_x, ragged_y):
                        _same(r, m.meanfield_prediction(xi, yi if with_y else None, **kw))
    assert eng.calls == 2 * 2 * 2 * 2 * 2


def test_refusals():
    g = load_golden("ilr_svi_dx2_dy1_k8")
    X, Y = g["X"], g["Y"]

    def model(affine=True):
        kind, ilr = mc.build_ilr(g, OracleEngine())
        ilr.init_transform(X, Y)
        ilr.models.likelihood.affine = affine
        return ilr
    eng = OracleBatchPredict()
    with pytest.raises(NotImplementedError):
        meanfield_prediction_batched([model()], X, dist='studentt', engine=eng)
    with pytest.raises(NotImplementedError):
        meanfield_prediction_batched([model()], X, prediction='median', engine=eng)
    with pytest.raises(NotImplementedError, match="affine"):
        meanfield_prediction_batched([model(), model(affine=False)], X, engine=eng)
    with pytest.raises(ValueError):
        meanfield_prediction_batched([], X, engine=eng)
    with pytest.raises(ValueError):
        meanfield_prediction_batched([model()], [X, X], engine=eng)
    with pytest.raises(ValueError):
        meanfield_prediction_batched([model(), model()], [X, X], Y, engine=eng)
    assert eng.calls == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_barrier_of_the_new_kernel_file_is_reached_with_lds_drained(tmp_path):
    asm = str(tmp_path / "mimo_predict_batched.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-fno-honor-nans",
           "-Wno-unused-function", "-S", "-o", asm, os.path.join(ROOT, "mimo_amd", "csrc", "mimo_predict_batched.hip")]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_barrier_waits as cbw
    kernels = cbw.kernels_of(asm)
    assert len(kernels) >= 64, "kernel symbols not found in the assembly"
    bad = {k: cbw.check(L) for k, L in kernels.items()}
    bad = {k: v for k, v in bad.items() if v}
    assert not bad, f"{len(bad)} kernels reach an s_barrier with LDS operations pending, e.g. {list(bad.items())[:3]}"
