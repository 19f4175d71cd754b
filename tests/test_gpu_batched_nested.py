"""GPU: the nested batch — B problems over ONE data set (mimo_upload_batched_shared), the weighted batched softmax pass
(mimo_estep_batched_weighted), the outer step on the device (mimo_outer_resp_batched, mimo_get_row_weights_batched) and the
nested mean-field driver of the mixtures of mixtures (mixtures/batched.py: meanfield_coordinate_descent_nested).

Reference: the NumPy oracle on each problem's rows alone (statistics of r * w; scalars and lse of the unweighted r), SciPy's
logsumexp for the outer step, a solo HipEngine pass, and the reference's own mixture-of-mixtures fixtures.  TOL and qerr are
the batched path's own (batched_checks).  What must hold bit for bit — a shared batch against a ragged batch of copies, unit
weights against the plain pass, a problem alone against the same problem in a batch, a repeated call, resident weights
against the same weights from the host — is compared with np.array_equal.

The per-row bound |sum_b w - 1| <= 1e-14 of the outer step: each w_b = e_b / s is one correctly rounded division (<= 2^-53
relative), and s is B - 1 sequential additions of terms <= 1 (<= (B - 1) 2^-53 relative); at B = 70 that is 70 * 1.1e-16 =
7.8e-15 at the very worst."""
import numpy as np
import numpy.random as npr
import pytest
from scipy.special import logsumexp

from batched_checks import TOL, ncb_of, MAX_D, oracle, pair_kmax, pair_of, problems, qerr, split
from conftest import load_golden, rel_err
from mimo_amd import _lib
from mimo_amd.batched import BatchedHipEngine
from mimo_amd.engine import HipEngine, _ptr
from mimo_amd.mixtures.batched import expected_responsibilities_nested, meanfield_coordinate_descent_nested
from oracle import mimo_oracle as O
from test_batched_nested_cpu import FIXTURES, _outer, posteriors

pytestmark = pytest.mark.gpu

SHARED_SHAPES = [(2, 4), (2, 100), (8, 64), (16, 47)]
SHARED_ROWS = [1, 33, 129, 520]            # one row, a one-row last tile, two workgroups, five workgroups
WEIGHTED_ROWS = (33, 0, 129, 1)
# one (Dz, K) per (NCB, RBW) pair: the largest Dz of the column-block count, the pair's largest K
WEIGHTED_CELLS = [(max(D for D in range(1, MAX_D + 1) if ncb_of(D) == ncb), pair_kmax(ncb, rbw))
                  for ncb in range(1, 11) for rbw in (1, 2) if pair_kmax(ncb, rbw)]
OUTER_B = [1, 2, 5, 70]
OUTER_N = [1, 255, 256, 257, 1000]


@pytest.fixture(scope="module")
def beng():
    return BatchedHipEngine(0)


@pytest.fixture(scope="module")
def beng2():
    return BatchedHipEngine(0)


@pytest.fixture(scope="module")
def solo():
    return HipEngine(0)


def packed(S):
    return np.stack([s.packed() for s in S])


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_the_tables_cover_what_they_claim():
    assert len(WEIGHTED_CELLS) == 18
    assert sorted(pair_of(D, K) for D, K in WEIGHTED_CELLS) == sorted(
        (ncb, rbw) for ncb in range(1, 11) for rbw in (1, 2) if pair_kmax(ncb, rbw))
    assert [len(split(n)) for n in SHARED_ROWS] == [1, 1, 2, 5]
    assert len(split(129)) == 2 and 129 % 32 == 1


# ---- 1. a shared batch returns the bits of a ragged batch of copies ----------------------------------------------------
def every_pass(eng, c, b, W, N, full):
    """{name: arrays} of the passes over the batch the engine holds (B problems of N rows)."""
    B, K = c.shape
    out = {}
    S, sc = eng.estep(c, b, W)
    out["plain"] = (packed(S), sc)
    S, sc = eng.estep(c, b, W, keep_lse=True, entropy_split=True)
    out["keep_lse"] = (packed(S), sc, np.stack(eng.get_lse()))
    S, sc = eng.estep(c, b, W, stats=False, entropy_split=True)
    out["no_stats"] = (sc,)
    if not full:
        return out
    rng = np.random.default_rng(17)
    sel = [rng.integers(0, N, size=n) for n in (40, 0, 200)]
    S, sc = eng.estep(c, b, W, rows=sel, entropy_split=True)
    out["rows"] = (packed(S), sc)
    labels, S = eng.gibbs_labels(c, b, W, seeds=[3, 4, 5], sweep=2)
    out["gibbs_philox"] = (np.stack(labels), packed(S), np.stack(eng.get_labels()), packed(eng.label_stats(None, K)))
    u = [rng.random(N) for _ in range(B)]
    labels, S = eng.gibbs_labels(c, b, W, u=u)
    out["gibbs_host_u"] = (np.stack(labels), packed(S))
    given = [rng.integers(0, K, size=N).astype(np.int32) for _ in range(B)]
    out["label_stats"] = (packed(eng.label_stats(given, K)),)
    tables = [rng.standard_normal((K, N)) for _ in range(B)]
    out["weighted_stats"] = (packed(eng.weighted_stats(tables)),)
    S = eng.random_resp_stats(K, [7, 8, 9])
    out["random_resp_stats"] = (packed(S), np.stack(eng.get_resp(K)), packed(eng.weighted_stats(None, K)))
    w = [rng.random(N) for _ in range(B)]
    S, sc = eng.estep(c, b, W, row_weights=w, keep_lse=True)
    out["weighted"] = (packed(S), sc, np.stack(eng.get_lse()), np.stack(eng.get_row_weights()))
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", SHARED_ROWS)
@pytest.mark.parametrize("D,K", SHARED_SHAPES)
def test_shared_equals_ragged_bit_for_bit(beng, D, K, N, B):
    rng = np.random.default_rng(1000 * D + 10 * K + N + B)
    Zs, c, b, W = problems(rng, [N] * B, D, K)
    Z = Zs[0]
    full = N == 129 and B == 3
    beng.upload([Z] * B)
    ref = every_pass(beng, c, b, W, N, full)
    beng.upload_shared(Z, B)
    assert np.array_equal(beng.row_off, np.arange(B + 1) * N)
    got = every_pass(beng, c, b, W, N, full)
    assert got.keys() == ref.keys()
    for name in ref:
        assert len(got[name]) == len(ref[name])
        for x, y in zip(got[name], ref[name]):
            assert x.shape == y.shape and same(x, y), name
    assert got["keep_lse"][2].shape == (B, N)
    # a plain upload leaves shared mode
    beng.upload([Z[:1]] * 2)
    with pytest.raises(_lib.MimoHipError):
        beng.outer_responsibilities(np.zeros(2))


# ---- 2. the weighted pass: every instantiation ------------------------------------------------------------------------------
def weighted_oracle(Z, c, b, W, w):
    """(n, sx, sxx) of r * w, and the batched oracle's (scalars, lse): those of the unweighted r."""
    L = O.canonical_eval(Z, c, b, W)
    r = np.exp(L - O.logsumexp(L, axis=0))
    n, sx, sxx = O.packed_stats(Z, r * w[None, :])
    return (n, sx, sxx) + tuple(oracle(Z, c, b, W)[3:])


def weighted_errs(S, sc, lse, ref):
    n, sx, sxx, scal, l = ref
    return {"n": qerr(S.n[:, None], np.asarray(n)[:, None]), "sx": qerr(S.sx, sx), "sxx": qerr(S.sxx, sxx),
            "scalars": qerr(sc, scal), "lse": qerr(lse, l)}


@pytest.mark.parametrize("D,K", WEIGHTED_CELLS)
def test_weighted_pass_every_instantiation(beng, beng2, solo, D, K):
    rng = np.random.default_rng(77 * D + K)
    rows = list(WEIGHTED_ROWS)
    Zs, c, b, W = problems(rng, rows, D, K)
    ws = [np.where(rng.random(n) < 0.2, 0.0, rng.random(n)) for n in rows]
    ws[2][:3] = [0.0, 1.0, 0.5]
    beng.upload(Zs)
    S, sc = beng.estep(c, b, W, row_weights=ws, keep_lse=True, entropy_split=True)
    lse = beng.get_lse()
    assert all(same(x, y) for x, y in zip(beng.get_row_weights(), ws))
    for i, Z in enumerate(Zs):
        errs = weighted_errs(S[i], sc[i], lse[i], weighted_oracle(Z, c[i], b[i], W[i], ws[i]))
        print(f"D={D} K={K} problem {i} ({len(Z)} rows) against the oracle", errs)
        assert max(errs.values()) <= TOL, errs
        off = np.flatnonzero(np.isneginf(c[i]))
        assert len(off) == 1
        assert np.all(S[i].n[off] < 1e-290) and np.all(np.abs(S[i].sx[off]) < 1e-290) and np.all(np.abs(S[i].sxx[off]) < 1e-290)
        if len(Z) == 0:
            assert not S[i].packed().any() and not sc[i, 0]
            continue
        solo.upload(Z)
        S1, sc1 = solo.estep(c[i], b[i], W[i], row_weights=ws[i], keep_lse=True, entropy_split=True)
        errs = weighted_errs(S[i], sc[i], lse[i], (S1.n, S1.sx, S1.sxx, sc1, solo.get_lse()))
        print(f"D={D} K={K} problem {i} ({len(Z)} rows) against the solo pass", errs)
        assert max(errs.values()) <= TOL, errs
    # determinism, and the resident weights are the weights
    for rw in (ws, 'resident'):
        S2, sc2 = beng.estep(c, b, W, row_weights=rw, keep_lse=True, entropy_split=True)
        assert same(packed(S2), packed(S)) and same(sc2, sc) and all(same(x, y) for x, y in zip(beng.get_lse(), lse))
    # without the table flags the scalars' split is NaN, the rest the same bits; without statistics the scalars stay
    S2, sc2 = beng.estep(c, b, W, row_weights='resident')
    assert same(packed(S2), packed(S)) and same(sc2[:, 0], sc[:, 0]) and np.isnan(sc2[:, 1:]).all()
    S2, sc2 = beng.estep(c, b, W, row_weights='resident', stats=False, entropy_split=True)
    assert S2 is None and same(sc2, sc)
    # unit weights: the plain pass, bit for bit
    Sp, scp = beng.estep(c, b, W, keep_lse=True, entropy_split=True)
    lsep = beng.get_lse()
    Su, scu = beng.estep(c, b, W, row_weights=[np.ones(n) for n in rows], keep_lse=True, entropy_split=True)
    assert same(packed(Su), packed(Sp)) and same(scu, scp) and all(same(x, y) for x, y in zip(beng.get_lse(), lsep))
    assert all(same(x, y) for x, y in zip(lsep, lse))           # (the weights never reach the normalisers)
    # independence: every non-empty problem alone, and in another order
    for i in (0, 2, 3):
        beng2.upload([Zs[i]])
        Sa, sca = beng2.estep(c[i:i + 1], b[i:i + 1], W[i:i + 1], row_weights=[ws[i]], keep_lse=True, entropy_split=True)
        assert same(Sa[0].packed(), S[i].packed()) and same(sca[0], sc[i]) and same(beng2.get_lse()[0], lse[i])
    order = [2, 3, 1, 0]
    beng2.upload([Zs[i] for i in order])
    Sa, sca = beng2.estep(c[order], b[order], W[order], row_weights=[ws[i] for i in order], entropy_split=True)
    assert same(packed(Sa), packed(S)[order]) and same(sca, sc[order])


def test_weighted_pass_on_a_shared_batch(beng, solo):
    rng = np.random.default_rng(5)
    N, B, D, K = 129, 3, 2, 4
    Zs, c, b, W = problems(rng, [N] * B, D, K, off=None)
    w = rng.random((B, N))
    beng.upload_shared(Zs[0], B)
    S, sc = beng.estep(c, b, W, row_weights=w, keep_lse=True)
    lse = beng.get_lse()
    solo.upload(Zs[0])
    for i in range(B):
        errs = weighted_errs(S[i], sc[i], lse[i], weighted_oracle(Zs[0], c[i], b[i], W[i], w[i]))
        assert max(errs.values()) <= TOL, errs
        S1, sc1 = solo.estep(c[i], b[i], W[i], row_weights=w[i], keep_lse=True)
        errs = weighted_errs(S[i], sc[i], lse[i], (S1.n, S1.sx, S1.sxx, sc1, solo.get_lse()))
        assert max(errs.values()) <= TOL, errs
    S2, sc2 = beng.estep(c, b, W, row_weights=list(w), keep_lse=True)
    assert same(packed(S2), packed(S)) and same(sc2, sc)


# ---- 3. the outer step -----------------------------------------------------------------------------------------------------
def gating_cases(rng, B):
    lg = np.log(rng.dirichlet(np.ones(B)))
    far = lg.copy()
    far[::2] += 800.0                                    # entries 800 apart: the maximum must be subtracted
    cases = {"random": lg, "800 apart": far}
    if B > 1:
        off = lg.copy()
        off[B // 2] = -np.inf
        cases["one -inf"] = off
    return cases


@pytest.mark.parametrize("N", OUTER_N)
@pytest.mark.parametrize("B", OUTER_B)
def test_outer_step(beng, B, N):
    rng = np.random.default_rng(31 * B + N)
    D, K = 2, 4
    Zs, c, b, W = problems(rng, [N] * B, D, K, off=None)
    Z = Zs[0]
    c += rng.standard_normal((B, 1)) * 3.0               # inner mixtures that fit the rows differently well
    beng.upload_shared(Z, B)
    beng.estep(c, b, W, stats=False, keep_lse=True)
    lse = np.stack(beng.get_lse())
    assert lse.shape == (B, N) and np.isfinite(lse).all()
    for name, lg in gating_cases(rng, B).items():
        counts, ll = beng.outer_responsibilities(lg)
        w = np.stack(beng.get_row_weights())
        t = lse + lg[:, None]
        l = logsumexp(t, axis=0)
        ref = np.exp(t - l)
        errs = {"w": qerr(w, ref), "counts": qerr(counts, ref.sum(axis=1)), "loglik": abs(ll - l.sum()) / max(abs(l.sum()), 1.0),
                "rows": float(np.abs(w.sum(axis=0) - 1.0).max())}
        print(f"B={B} N={N} {name}", errs)
        assert max(errs["w"], errs["counts"], errs["loglik"]) <= TOL, (name, errs)
        assert errs["rows"] <= 1e-14, (name, errs)
        assert w.shape == (B, N) and np.all(w >= 0.0)
        assert np.all(w[np.isneginf(lg)] == 0.0)         # a switched-off problem: weights exactly 0
        # two calls: identical bits
        counts2, ll2 = beng.outer_responsibilities(lg)
        assert same(counts2, counts) and ll2 == ll and same(np.stack(beng.get_row_weights()), w)
        # the next pass reads these weights: the same pass with them given from the host, bit for bit
        Sr, scr = beng.estep(c, b, W, row_weights='resident', keep_lse=True)
        assert same(np.stack(beng.get_row_weights()), w)
        Sh, sch = beng.estep(c, b, W, row_weights=w, keep_lse=True)
        assert same(packed(Sr), packed(Sh)) and same(scr, sch)
        assert same(np.stack(beng.get_lse()), lse)
        errs = {"n": qerr(packed(Sr)[:, :, 0].sum(axis=1), counts)}      # sum_k n_k = sum_n w_n: the counts again
        assert errs["n"] <= TOL, errs
    if B == 1:
        with pytest.raises((ValueError, _lib.MimoHipError)):
            beng.outer_responsibilities(np.array([-np.inf]))


# ---- 4. errors, with the context usable afterwards ---------------------------------------------------------------------------
def test_errors_leave_the_context_usable(beng):
    rng = np.random.default_rng(9)
    N, B, D, K = 40, 2, 2, 4
    Zs, c, b, W = problems(rng, [N] * B, D, K)
    Z = Zs[0]
    lib, ctx = beng._lib, beng._ctx

    def usable():
        S, sc = beng.estep(c, b, W)
        assert np.isfinite(sc[:, 0]).all()
        return packed(S)
    beng.upload([Z, Z])
    ref = usable()
    beng.estep(c, b, W, stats=False, keep_lse=True)
    with pytest.raises(_lib.MimoHipError):                      # the outer step needs a shared batch
        beng.outer_responsibilities(np.zeros(B))
    with pytest.raises(_lib.MimoHipError):                      # no weights are resident after an upload
        beng.estep(c, b, W, row_weights='resident')
    with pytest.raises(_lib.MimoHipError):
        beng.get_row_weights()
    assert same(usable(), ref)
    beng.upload_shared(Z, B)
    with pytest.raises(_lib.MimoHipError):                      # no kept lse
        beng.outer_responsibilities(np.zeros(B))
    with pytest.raises(_lib.MimoHipError):
        beng.estep(c, b, W, row_weights='resident')
    beng.estep(c, b, W, stats=False, keep_lse=True)
    beng.estep(c, b, W)                                         # a pass without keep_lse ends the lse's residency
    with pytest.raises(_lib.MimoHipError):
        beng.outer_responsibilities(np.zeros(B))
    beng.estep(c, b, W, stats=False, keep_lse=True)
    for lg in (np.array([0.0, np.nan]), np.array([-np.inf, -np.inf]), np.array([np.inf, 0.0])):
        with pytest.raises(ValueError):
            beng.outer_responsibilities(lg)
        out = np.empty(B + 1)                                    # ... and the library's own check behind the Python one
        assert lib.mimo_outer_resp_batched(ctx, _ptr(lg), 0, _ptr(out)) == _lib.E_INVALID
    for w in ([np.ones(N), np.full(N, np.nan)], [np.ones(N), -np.ones(N)]):
        with pytest.raises(ValueError):
            beng.estep(c, b, W, row_weights=w)
        flat, S, sc = np.concatenate(w), np.empty((B, K, 1 + D + D * D)), np.empty((B, 3))
        assert lib.mimo_estep_batched_weighted(ctx, _ptr(c), _ptr(b), _ptr(W), K, _ptr(flat), 0, _ptr(S), _ptr(sc)) == _lib.E_INVALID
    with pytest.raises(ValueError):
        beng.estep(c, b, W, row_weights=[np.ones(N)] * B, rows=[np.arange(3)] * B)
    with pytest.raises(ValueError):
        beng.upload_shared(np.zeros((0, D)), B)
    z = np.zeros((1, D))
    assert lib.mimo_upload_batched_shared(ctx, _ptr(z), 0, B, D) == _lib.E_INVALID
    assert lib.mimo_upload_batched_shared(ctx, _ptr(z), 1, 0, D) == _lib.E_INVALID
    bad = Z.copy()
    bad[3, 1] = np.nan
    with pytest.raises(_lib.MimoHipError):
        beng.upload_shared(bad, B)
    # after all of it: the lse kept before the refused calls is still there, and a fresh upload gives the first bits
    counts, _ = beng.outer_responsibilities(np.log([0.25, 0.75]))
    assert abs(counts.sum() - N) <= 1e-12 * N
    beng.upload_shared(Z, B)
    assert same(usable(), ref)


# ---- 5. the nested driver against the reference's fixtures and the solo driver -------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_nested_driver_against_the_reference_fixture(name):
    g = load_golden(name)
    solo = HipEngine(0)             # (its own engine: the tied inner mixtures bind it under the 'linear' structure)
    X, seed = g["X"], int(g["seed"])
    npr.seed(seed + 6)
    mm = _outer(g, solo)
    npr.seed(seed + 7)
    meanfield_coordinate_descent_nested(mm, X, randomize=True, maxiter=3, maxsubiter=2, maxsubsubiter=2)
    got = posteriors(mm)
    errs = {key: rel_err(v, g["mom_vi_" + key]) for key, v in got.items()}
    errs["resp"] = rel_err(expected_responsibilities_nested(mm, X), g["mom_vi_resp"])
    print(name, "against the fixture", errs)
    assert max(errs.values()) < 1e-7, errs

    npr.seed(seed + 6)
    ref = _outer(g, solo)
    npr.seed(seed + 7)
    ref.meanfield_coordinate_descent(X, randomize=True, maxiter=3, maxsubiter=2, maxsubsubiter=2, progress_bar=False)
    errs = {key: rel_err(got[key], v) for key, v in posteriors(ref).items()}
    errs["resp"] = rel_err(expected_responsibilities_nested(mm, X), ref.expected_responsibilities(X))
    print(name, "against the solo driver", errs)
    assert max(errs.values()) < 1e-8, errs
