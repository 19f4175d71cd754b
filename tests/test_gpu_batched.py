"""GPU: the batched softmax pass (mimo_upload_batched / mimo_estep_batched, mimo_amd.batched.BatchedHipEngine) against
B solo passes, the oracle and the reference fixtures; independence and determinism; loud failures."""

import numpy as np
import pytest
from scipy.special import logsumexp

from batched_checks import TOL, check_against, oracle, problems, qerr
from conftest import load_golden
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.engine import HipEngine, _ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def beng():
    return BatchedHipEngine(0)


@pytest.fixture(scope="module")
def solo():
    return HipEngine(0)


CASES = [  # (rows, Dz, K)
    ([4099], 2, 4),
    ([0, 33, 31], 1, 1),
    ([0, 1, 31, 32, 33, 4099], 1, 4),
    ([4099, 0, 1, 31, 32, 33], 2, 50),
    ([33, 4099, 0, 1, 31, 32], 2, 128),
    ([1, 0, 4099, 32], 2, 100),
    ([31, 32, 4099, 0, 1, 33], 11, 128),
    ([32, 4099, 1], 11, 4),
    ([0, 1, 31, 32, 33, 4099], 11, 50),
    ([4099, 33, 0, 1], 16, 64),
    ([1, 32, 31], 16, 1),
]


@pytest.mark.parametrize("rows,D,K", CASES)
def test_batched_equals_solo_and_oracle(beng, solo, rows, D, K):
    rng = np.random.default_rng(100 * D + K + len(rows))
    Zs, c, b, W = problems(rng, rows, D, K)
    beng.upload(Zs)
    Sb, scb = beng.estep(c, b, W, keep_lse=True, entropy_split=True)
    lseb = beng.get_lse()
    for i, Z in enumerate(Zs):
        check_against(Sb[i], scb[i], lseb[i], oracle(Z, c[i], b[i], W[i]))
        if len(Z) == 0:
            continue
        solo.upload(Z)
        S1, sc1 = solo.estep(c[i], b[i], W[i], keep_lse=True, entropy_split=True)
        check_against(Sb[i], scb[i], lseb[i], (S1.n, S1.sx, S1.sxx, sc1, solo.get_lse()))
    # without the split the two entropy scalars are NaN, without statistics only the scalars come back
    S2, sc2 = beng.estep(c, b, W)
    assert np.array_equal(sc2[:, 0], scb[:, 0]) and np.isnan(sc2[:, 1:]).all()
    assert all(np.array_equal(x.sxx, y.sxx) for x, y in zip(S2, Sb))
    S3, sc3 = beng.estep(c, b, W, stats=False, entropy_split=True)
    assert S3 is None and np.array_equal(sc3, scb)


def test_many_tiny_problems(beng):
    rng = np.random.default_rng(7)
    rows = list(rng.integers(0, 41, size=300))
    Zs, c, b, W = problems(rng, rows, 2, 4)
    beng.upload(Zs)
    Sb, scb = beng.estep(c, b, W, keep_lse=True, entropy_split=True)
    lseb = beng.get_lse()
    for i, Z in enumerate(Zs):
        check_against(Sb[i], scb[i], lseb[i], oracle(Z, c[i], b[i], W[i]))


def _fixture_pair(names, build):
    gs = [load_golden(n) for n in names]
    rows, params, refs = [], [], []
    for g in gs:
        Z, theta, ref = build(g)
        rows.append(Z); params.append(theta); refs.append(ref)
    c, b, W = (np.stack([p[i] for p in params]) for i in range(3))
    return rows, (c, b, W), refs


def _gmm(g):
    from model_checks import build_gmm, load_gmm_state
    kind, model = build_gmm(g, None)
    load_gmm_state(model, g, kind)
    ref = (g["counts"], g["stats_xk"], g["stats_xxTk"], g["vlb_obs"] + g["vlb_labels"], g["A4_ell"], g["A4_elcl"], g["A4_eresp"])
    return g["X"], model.canonical_expected(), ref


def _ilr(g):
    from model_checks import build_ilr, load_ilr_state
    from mimo_amd.distributions.lingauss import joint_rows
    kind, ilr = build_ilr(g, None)
    load_ilr_state(ilr, g, kind)
    Z = np.asarray(joint_rows(g["X"], g["Y"]))
    # the fixture's expected log-likelihood per row: logsumexp_k of its expected log complete likelihood
    ell = logsumexp(g["A7_elcl"], axis=0)
    ref = (g["counts"], g["mstats_yxTk"], g["mstats_yyTk"], g["vlb_data"] + g["vlb_labels"], ell, g["A7_elcl"], g["A7_eresp"])
    return Z, ilr.canonical_expected(), ref


@pytest.mark.parametrize("names,kind", [
    (("gmm_c2_d16_k16_dir", "gmm_c2_d16_k16_n4099"), "gmm"),
    (("gmm_c3_d8_k32_stick", "gmm_c3_d8_k32_n4099"), "gmm"),
    (("ilr_dx1_dy1_k50_stick", "ilr_dx1_dy1_k50_n4099"), "ilr"),
])
def test_reference_fixtures(beng, names, kind):
    rows, (c, b, W), refs = _fixture_pair(names, _gmm if kind == "gmm" else _ilr)
    beng.upload(rows)
    S, sc = beng.estep(c, b, W, keep_lse=True)
    lse = beng.get_lse()
    tol = 1e-9
    for i, (n, s1, s2, vlb, ell, elcl, eresp) in enumerate(refs):
        assert qerr(S[i].n[:, None], n[:, None]) < tol
        assert abs(sc[i, 0] - vlb) < tol * abs(vlb)
        assert qerr(lse[i], ell) < tol
        # responsibilities: the fixture's expected log complete likelihood normalised by the pass's lse rows
        assert np.abs(np.exp(elcl - lse[i][None, :]) - eresp).max() < tol
        if kind == "gmm":
            assert qerr(S[i].sx, s1) < tol and qerr(S[i].sxx, s2) < tol
        else:          # z = [x, y]: sum r y x~' = the (y, [x, 1]) blocks, sum r y y' the (y, y) block
            dx = rows[i].shape[1] - 1
            yx = np.concatenate([S[i].sxx[:, dx:, :dx], S[i].sx[:, dx:, None]], axis=2)
            assert qerr(yx, s1) < tol and qerr(S[i].sxx[:, dx:, dx:], s2) < tol


def test_independence_and_determinism(beng):
    rng = np.random.default_rng(11)
    Zs, c, b, W = problems(rng, [4099, 1000, 33], 8, 32)
    beng.upload(Zs)
    S0, sc0 = beng.estep(c, b, W, keep_lse=True)
    l0 = beng.get_lse()
    S1, sc1 = beng.estep(c, b, W, keep_lse=True)          # two runs: bit-identical
    assert np.array_equal(sc0, sc1) and all(np.array_equal(x.packed(), y.packed()) for x, y in zip(S0, S1))
    assert all(np.array_equal(x, y) for x, y in zip(l0, beng.get_lse()))
    # problem 0's data (and row count) and parameters change: problem 1 and 2 do not move by a bit
    Zs2 = [rng.standard_normal((777, 8))] + Zs[1:]
    c2, b2, W2 = c.copy(), b.copy(), W.copy()
    c2[0] += 1.0; b2[0] *= 0.5; W2[0] *= 2.0
    beng.upload(Zs2)
    S2, sc2 = beng.estep(c2, b2, W2, keep_lse=True)
    l2 = beng.get_lse()
    for i in (1, 2):
        assert np.array_equal(S2[i].packed(), S0[i].packed()) and np.array_equal(sc2[i], sc0[i]) and np.array_equal(l2[i], l0[i])
    # a problem alone and in a batch of identical copies: the same bits
    beng.upload([Zs[1]])
    Sa, sca = beng.estep(c[1:2], b[1:2], W[1:2])
    beng.upload([Zs[1]] * 5)
    Sc, scc = beng.estep(np.repeat(c[1:2], 5, 0), np.repeat(b[1:2], 5, 0), np.repeat(W[1:2], 5, 0))
    for i in range(5):
        assert np.array_equal(Sc[i].packed(), Sa[0].packed()) and np.array_equal(scc[i, 0], sca[0, 0])
        assert np.array_equal(Sc[i].packed(), S0[1].packed()) and np.array_equal(scc[i, 0], sc0[1, 0])


def test_unsupported_shapes_fail_loudly(beng):
    rng = np.random.default_rng(5)
    with pytest.raises(_lib.MimoHipError):
        beng.upload([rng.standard_normal((40, 17))])
    for D, K in ((16, 65), (2, 129)):
        Zs, c, b, W = problems(rng, [40, 3], D, K)
        beng.upload(Zs)
        with pytest.raises(_lib.MimoHipError):
            beng.estep(c, b, W)
    Zs, c, b, W = problems(rng, [40, 3], 3, 4)
    beng.upload(Zs)
    beng.set_structure('diag')
    try:
        with pytest.raises(_lib.MimoHipError):
            beng.estep(c, b, W * np.eye(3))
    finally:
        beng.set_structure('full')


def test_mode_errors(beng, solo):
    rng = np.random.default_rng(6)
    Zs, c, b, W = problems(rng, [40, 3], 3, 4)
    beng.upload(Zs)
    lib, ctx = beng._lib, beng._ctx
    S = np.empty((4, 13)); sc = np.empty(3); lab = np.empty(43, dtype=np.int32)
    # single-problem entry points on a batched context
    assert lib.mimo_estep(ctx, _ptr(c[0]), _ptr(b[0]), _ptr(W[0]), 4, 0, _ptr(S), _ptr(sc)) == _lib.E_INVALID
    assert b"batch" in lib.mimo_last_error(ctx)
    assert lib.mimo_gibbs_labels(ctx, _ptr(c[0]), _ptr(b[0]), _ptr(W[0]), 4, 1, 0, None, 0, _ptr(lab), _ptr(S)) == _lib.E_INVALID
    assert lib.mimo_label_stats(ctx, _ptr(lab), 4, 0, _ptr(S)) == _lib.E_INVALID
    # a plain upload returns the context to single-problem mode, and the batched pass then refuses
    Z = np.ascontiguousarray(Zs[0])
    assert lib.mimo_upload(ctx, _ptr(Z), len(Z), 3) == 0
    c0 = np.ascontiguousarray(c[0]); b0 = np.ascontiguousarray(b[0]); W0 = np.ascontiguousarray(W[0])
    assert lib.mimo_estep(ctx, _ptr(c0), _ptr(b0), _ptr(W0), 4, 0, _ptr(S), _ptr(sc)) == 0
    S2 = np.empty((2, 4, 13)); sc2 = np.empty((2, 3))
    assert lib.mimo_estep_batched(ctx, _ptr(c), _ptr(b), _ptr(W), 4, 0, _ptr(S2), _ptr(sc2)) == _lib.E_INVALID
    solo.upload(Z)
    assert lib.mimo_estep_batched(solo._ctx, _ptr(c), _ptr(b), _ptr(W), 4, 0, _ptr(S2), _ptr(sc2)) == _lib.E_INVALID
    # non-finite rows, non-finite parameters, parameter shapes
    for bad in (np.nan, np.inf):
        Zb = [Zs[0].copy(), Zs[1]]
        Zb[0][5, 1] = bad
        with pytest.raises(_lib.MimoHipError):
            beng.upload(Zb)
    beng.upload(Zs)
    for name, val in (("c", np.nan), ("c", np.inf), ("b", np.nan), ("W", np.inf)):
        p = {"c": c.copy(), "b": b.copy(), "W": W.copy()}
        p[name].flat[3] = val
        with pytest.raises(_lib.MimoHipError):
            beng.estep(p["c"], p["b"], p["W"])
    with pytest.raises(ValueError):
        beng.estep(c[:1], b[:1], W[:1])
    with pytest.raises(ValueError):
        beng.estep(c, b[:, :, :2], W)
    with pytest.raises(ValueError):
        beng.estep(c, b, W[:, :3])
    # the pass still runs after all of that
    S, sc = beng.estep(c, b, W)
    assert np.isfinite(sc[:, 0]).all()
